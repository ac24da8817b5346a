"""The steps that sit immediately before the forward path in the reference's data pipeline
(SURVEY.md section 8f, rank 1), in two forms:

* host mirrors with the reference's names and semantics (`uniform_temporal_subsample`,
  `uniform_temporal_subsample_repeated`, `div_255`, `Normalize`, `Div255`: reference
  pytorchvideo/transforms/functional.py:19-41,134-160 and transforms/transforms.py:177-195,414-430),
  so existing pipelines keep working, and
* `DevicePacker`: the same arithmetic fused into the MI355X deploy form's ingest kernel
  (`pv_ingest_ncdhw`): a decoded uint8 (or float) clip [B,3,T,H,W] that is already on the device --
  or is uploaded once, as the fast-rate clip only -- is frame-subsampled per pathway, scaled,
  normalised, converted to bf16 and laid out channels-last in ONE pass per pathway.  The reference
  does this as index_select + div + sub + div on the host followed by an upload of every pathway.

The spatial half of the eval protocol -- `short_side_scale` then `uniform_crop` (functional.py:92-131,302-347;
transforms.py:100-121,153-175), with their box variants -- has the same two forms: host mirrors, and
`DevicePacker(..., short_side=, crop_size=, spatial_idx=)` / `device_scale_crop`, which run it inside the same pass
(`pv_resample_crop`): the clip may then have any frame size, and one launch per pathway turns it into the crops.

Decoder-native frames -- YUV 4:2:0 as NV12 / NV21 (what a GPU decoder writes) or I420 / YV12 (a CPU decoder's yuv420p) -- are
a source layout of that same pass (`pv_yuv_views`): `yuv_matrix` composes the conversion, `yuv420_to_rgb` is the host mirror
of the tap rule, and `device_scale_crop` / `DevicePacker` / `inference.VideoPredictor` take `src_layout="NV12"` and friends.

HDR streams -- most 10-bit footage: a phone's HLG, HDR10 / AV1 PQ -- give BT.2020 R'G'B' under a PQ or HLG curve, which a
network trained on BT.709 SDR misreads.  `hdr="pq"` / `"hlg"` / `(transfer, tone_params(...))` on `device_scale_crop`,
`DevicePacker` and the predictors maps every tap to SDR inside the same launch (`pv_hdr_views`); `hdr_to_sdr` is the host
mirror, composed with `yuv420_to_rgb`.

Many videos per forward: `DevicePacker.video_batch` + `fill_batch` give every item of the deploy batch a source of its own
(`pv_batch_views`), so that the views of videos of any lengths and frame sizes share a forward (`inference.VideoBatchPredictor`).

Key-frame detection: a detection form takes the same batch path (`keyframes=True`) -- rectangular and uncropped with
`short_side` alone, the detection tutorial's protocol -- and `DevicePacker.fill_boxes` maps the boxes of a forward from the
pixels of their source frames into the views on the device (`pv_box_views`); `boxes_to_view` is the host mirror, composed of
the box mirrors above, and `inference.KeyframeDetector` the loop around it.
"""
import copy
import math
import operator
from typing import Dict, Sequence, Tuple

import torch


# --------------------------------------------------------------------------- host mirrors
def uniform_temporal_subsample(x: torch.Tensor, num_samples: int, temporal_dim: int = -3) -> torch.Tensor:
    """transforms/functional.py:19-41: `num_samples` equispaced frames (nearest neighbour when
    num_samples exceeds the clip length)."""
    t = x.shape[temporal_dim]
    assert num_samples > 0 and t > 0
    return torch.index_select(x, temporal_dim, temporal_indices(t, num_samples).to(x.device))


def temporal_indices(t: int, num_samples: int) -> torch.Tensor:
    """The frame indices uniform_temporal_subsample selects (int64)."""
    return torch.clamp(torch.linspace(0, t - 1, num_samples), 0, t - 1).long()


def uniform_temporal_subsample_repeated(frames: torch.Tensor, frame_ratios: Sequence[int],
                                        temporal_dim: int = -3) -> Tuple[torch.Tensor, ...]:
    """transforms/functional.py:134-160: one subsampled copy per pathway (SlowFast: ratios (4, 1))."""
    t = frames.shape[temporal_dim]
    return [uniform_temporal_subsample(frames, t // r, temporal_dim) for r in frame_ratios]


def div_255(x: torch.Tensor) -> torch.Tensor:
    """transforms/functional.py div_255: [0,255] -> [0,1]."""
    return x / 255.0


class Div255(torch.nn.Module):
    def forward(self, x):
        return div_255(x)


class Normalize(torch.nn.Module):
    """transforms/transforms.py:177-195: per-channel (x - mean) / std of a (C,T,H,W) or (B,C,T,H,W) clip."""

    def __init__(self, mean, std):
        super().__init__()
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)

    def forward(self, x):
        shape = [1] * x.dim()
        shape[-4] = len(self.mean)
        mean = torch.tensor(self.mean, dtype=x.dtype, device=x.device).view(shape)
        std = torch.tensor(self.std, dtype=x.dtype, device=x.device).view(shape)
        return (x - mean) / std


# --------------------------------------------------------------------------- spatial host mirrors
def scaled_size(h: int, w: int, size: int) -> Tuple[int, int]:
    """The (new_h, new_w) short_side_scale resizes an h x w frame to (functional.py:121-126: the long side is floored)."""
    if w < h:
        return int(math.floor((float(h) / w) * size)), size
    return size, int(math.floor((float(w) / h) * size))


def crop_offsets(new_h: int, new_w: int, size: int, spatial_idx: int) -> Tuple[int, int]:
    """The (y, x) origin of uniform_crop's window (functional.py:311-323: centred with ceil; index 0 / 2 move it to the
    start / end of the LONGER side)."""
    assert spatial_idx in [0, 1, 2]
    y = int(math.ceil((new_h - size) / 2))
    x = int(math.ceil((new_w - size) / 2))
    if new_h > new_w:
        if spatial_idx == 0:
            y = 0
        elif spatial_idx == 2:
            y = new_h - size
    else:
        if spatial_idx == 0:
            x = 0
        elif spatial_idx == 2:
            x = new_w - size
    return y, x


def short_side_scale(x: torch.Tensor, size: int, interpolation: str = "bilinear", backend: str = "pytorch") -> torch.Tensor:
    """functional.py:92-131: scale the shorter side of a (C,T,H,W) float32 clip to `size`, keeping the aspect ratio."""
    assert len(x.shape) == 4
    assert x.dtype == torch.float32
    assert backend in ("pytorch", "opencv")
    if backend != "pytorch":
        raise NotImplementedError("%s backend not supported." % backend)
    _, _, h, w = x.shape
    # torch takes align_corners with the interpolating modes only; "area" and "nearest" have no corners to align (the
    # reference passes False for every mode, which torch refuses for these two)
    corners = False if interpolation in ("linear", "bilinear", "bicubic", "trilinear") else None
    return torch.nn.functional.interpolate(x, size=scaled_size(h, w, size), mode=interpolation, align_corners=corners)


def uniform_crop(images: torch.Tensor, size: int, spatial_idx: int) -> torch.Tensor:
    """functional.py:326-347: the left / centre / right (top / centre / bottom for a portrait clip) size x size crop."""
    y, x = crop_offsets(images.shape[2], images.shape[3], size, spatial_idx)
    return images[:, :, y: y + size, x: x + size]


def clip_boxes_to_image(boxes: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """functional.py:407-426: clip [N,4] boxes (x1, y1, x2, y2) to a height x width image."""
    clipped = copy.deepcopy(boxes)
    clipped[:, [0, 2]] = torch.clamp(boxes[:, [0, 2]], 0.0, width - 1.0)
    clipped[:, [1, 3]] = torch.clamp(boxes[:, [1, 3]], 0.0, height - 1.0)
    return clipped


def crop_boxes(boxes: torch.Tensor, x_offset: int, y_offset: int) -> torch.Tensor:
    """functional.py:429-446: boxes in the coordinates of a crop whose origin is (x_offset, y_offset)."""
    cropped = copy.deepcopy(boxes)
    cropped[:, [0, 2]] = boxes[:, [0, 2]] - x_offset
    cropped[:, [1, 3]] = boxes[:, [1, 3]] - y_offset
    return cropped


def short_side_scale_with_boxes(images: torch.Tensor, boxes: torch.Tensor, size: int, interpolation: str = "bilinear",
                                backend: str = "pytorch") -> Tuple[torch.Tensor, torch.Tensor]:
    """functional.py:195-231: short_side_scale, and the boxes scaled by the ratio of the LONGER side (in place, as there)."""
    _, _, h, w = images.shape
    images = short_side_scale(images, size, interpolation, backend)
    _, _, new_h, new_w = images.shape
    if w < h:
        boxes *= float(new_h) / h
    else:
        boxes *= float(new_w) / w
    return images, boxes


def uniform_crop_with_boxes(images: torch.Tensor, size: int, spatial_idx: int,
                            boxes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """functional.py:350-378: uniform_crop, and the boxes moved into the crop and clipped to it."""
    y, x = crop_offsets(images.shape[2], images.shape[3], size, spatial_idx)
    cropped = images[:, :, y: y + size, x: x + size]
    return cropped, clip_boxes_to_image(crop_boxes(boxes, x, y), cropped.shape[-2], cropped.shape[-1])


def orientation_code(rotation: int = 0, mirror: bool = False) -> int:
    """The `orient` code of a `pv_view_source` record (include/pv_mi355x.h): `rotation` is the clockwise turn the stream's
    metadata asks for -- 0, 90, 180 or 270 degrees, a decoder's "rotate 90" -- and `mirror` the horizontal flip of the turned
    frame (a front camera): rot | (mirror << 2)."""
    if isinstance(rotation, bool) or rotation not in (0, 90, 180, 270):
        raise ValueError("rotation is 0, 90, 180 or 270 degrees clockwise, got %r" % (rotation,))
    return int(rotation) // 90 | (4 if mirror else 0)


def _orient(code, what="orientation"):
    try:
        if isinstance(code, bool):
            raise TypeError
        code = operator.index(code)                  # any integer type: int, numpy, a 0-d tensor
    except TypeError:
        raise ValueError("%s is a code 0..7 (orientation_code), got %r" % (what, code)) from None
    if not 0 <= code <= 7:
        raise ValueError("%s is a code 0..7 (orientation_code), got %d" % (what, code))
    return code


def displayed_size(height: int, width: int, orient: int) -> Tuple[int, int]:
    """(Hd, Wd) of a stored height x width frame under `orient`: a quarter turn swaps the two."""
    return (width, height) if _orient(orient) & 1 else (height, width)


def oriented(x: torch.Tensor, orient: int, h_dim: int = -2, w_dim: int = -1) -> torch.Tensor:
    """The displayed frame(s) of stored frame(s) `x` under `orient`, the host mirror of the ingest's rule:
    `torch.rot90(x, -rot, (h_dim, w_dim))`, then `.flip(w_dim)` if the mirror bit is set.  The result is a view or a copy as
    torch decides; call `.contiguous()` for a dense one."""
    orient = _orient(orient)
    if orient & 3:
        x = torch.rot90(x, -(orient & 3), (h_dim, w_dim))
    return x.flip(w_dim) if orient & 4 else x


def orient_boxes(boxes: torch.Tensor, height: int, width: int, orient: int) -> torch.Tensor:
    """fp32 [N,4] boxes (x1, y1, x2, y2) in the pixels of a STORED height x width frame -> the same boxes in the pixels of the
    displayed frame, the host mirror of `pv_box_views`: every operation rounded on its own in fp32.  A mirrored coordinate
    along an axis of stored length n is `n - v - 1` in that order (the reference's `horizontal_flip_with_boxes`,
    functional.py:380-404, which code 4 equals), a quarter turn swaps x and y, and the corners are re-ordered so that
    x1 <= x2 and y1 <= y2.  The input is not modified."""
    orient = _orient(orient)
    b = boxes.detach().to("cpu", torch.float32).clone()
    if orient == 0:
        return b
    x, y = b[:, [0, 2]], b[:, [1, 3]]

    def mirror(v, n):
        return (float(n) - v) - 1.0

    rot = orient & 3
    if rot == 1:
        x, y = mirror(y, height), x
    elif rot == 2:
        x, y = mirror(x, width), mirror(y, height)
    elif rot == 3:
        x, y = y, mirror(x, width)
    if orient & 4:
        x = mirror(x, displayed_size(height, width, orient)[1])
    out = torch.empty_like(b)
    out[:, 0], out[:, 2] = torch.minimum(x[:, 0], x[:, 1]), torch.maximum(x[:, 0], x[:, 1])
    out[:, 1], out[:, 3] = torch.minimum(y[:, 0], y[:, 1]), torch.maximum(y[:, 0], y[:, 1])
    return out


def boxes_to_view(boxes: torch.Tensor, height: int, width: int, short_side: int, crop_size=None, spatial_idx: int = 1,
                  clip_to_source: bool = False, orientation: int = 0) -> torch.Tensor:
    """The host mirror of `pv_box_views` (include/pv_mi355x.h): fp32 [N,4] boxes (x1, y1, x2, y2) in the pixels of a
    height x width SOURCE frame -> the same boxes in the pixels of the view the ingest cuts from that frame, composed from the
    mirrors above in the reference's order: `clip_boxes_to_image` to the source (`clip_to_source`: the detection tutorial's
    first step), `short_side_scale_with_boxes`, then `crop_boxes` to the origin of the `crop_size` window of `spatial_idx`
    -- `crop_size=None`: no crop, the window is the whole scaled frame -- and `clip_boxes_to_image` to the window.  The
    input is not modified.  Boxes are finite.  `orientation` (`orientation_code`): `height` x `width` and the boxes are the
    STORED frame's; behind the first clip the boxes go into the displayed frame (`orient_boxes`), whose size the scale and
    the crop then see."""
    out = boxes.detach().to("cpu", torch.float32).clone()
    if clip_to_source:
        out = clip_boxes_to_image(out, height, width)
    if _orient(orientation):
        out = orient_boxes(out, height, width, orientation)
        height, width = displayed_size(height, width, orientation)
    frame = torch.zeros(1, dtype=torch.float32).expand(1, 1, height, width)          # only its size is used
    scaled, out = short_side_scale_with_boxes(frame, out, short_side)
    hn, wn = scaled.shape[-2:]
    if crop_size is None:
        return clip_boxes_to_image(out, hn, wn)
    if crop_size > hn or crop_size > wn:
        raise RuntimeError("a %d crop does not fit the %d x %d frame scaled to %d x %d" % (crop_size, height, width, hn, wn))
    y, x = crop_offsets(hn, wn, crop_size, spatial_idx)
    return clip_boxes_to_image(crop_boxes(out, x, y), crop_size, crop_size)


def _size_pair(size, what="size"):
    """(Ho, Wo) of an int or a pair, both positive."""
    ho, wo = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size), int(size))
    if ho < 1 or wo < 1 or (isinstance(size, (tuple, list)) and len(size) != 2):
        raise ValueError("%s is a positive int or a pair (Ho, Wo); got %r" % (what, size))
    return ho, wo


def _check_regions(regions, height, width, even=False, what="regions"):
    """`regions` as a host int64 tensor [..., 4] of (top, left, h, w), every rectangle at least 1 x 1 and inside the
    height x width frame -- and, `even`, of even members (YUV 4:2:0: a chroma sample is never split; `even="width"`, YUV
    4:2:2: left and w only).  ValueError otherwise."""
    regions = torch.as_tensor(regions)
    if regions.dim() < 1 or regions.shape[-1] != 4 or regions.numel() == 0 or regions.is_floating_point() or regions.dtype == torch.bool:
        raise ValueError("%s are integer (top, left, h, w) rectangles [..., 4]; got %s %s" % (what, regions.dtype, tuple(regions.shape)))
    regions = regions.detach().to("cpu", torch.int64)
    top, left, h, w = regions.unbind(-1)
    if bool((h < 1).any()) or bool((w < 1).any()):
        raise ValueError("%s: a rectangle is at least 1 x 1" % what)
    if bool((top < 0).any()) or bool((left < 0).any()) or bool((top + h > height).any()) or bool((left + w > width).any()):
        raise ValueError("%s: a rectangle leaves the %d x %d frame" % (what, height, width))
    if even == "width":
        if bool((regions[..., 1::2] % 2 != 0).any()):
            raise ValueError("%s: the rectangles of a YUV 4:2:2 source have even left and w (box_regions(..., even='width'))" % what)
    elif even and bool((regions % 2 != 0).any()):
        raise ValueError("%s: the rectangles of a YUV 4:2:0 source have even top, left, h and w (box_regions(..., even=True))" % what)
    return regions


def resized_crop(frames: torch.Tensor, regions, size) -> torch.Tensor:
    """The deterministic core of the reference's `random_resized_crop` (transforms/functional.py): rows
    [top, top + h) x columns [left, left + w) of every frame, resized to `size` by
    `interpolate(mode="bilinear", align_corners=False)`, frame by frame.  `frames` is (C, T, H, W); `regions` an integer
    (top, left, h, w) -- one rectangle for the clip -- or [T, 4], one per frame (what `shift=True` builds); `size` an int or
    (Ho, Wo).  Returns (C, T, Ho, Wo) fp32.  Every tap stays inside the rectangle: this is crop, then resize, not a window of
    the resized frame.  The host mirror of `device_resized_crop` / `pv_region_views`."""
    if frames.dim() != 4:
        raise ValueError("frames are (C, T, H, W); got %s" % (tuple(frames.shape),))
    c, t, height, width = frames.shape
    ho, wo = _size_pair(size)
    regions = _check_regions(regions, height, width)
    if regions.dim() == 1:
        regions = regions.expand(t, 4)
    if tuple(regions.shape) != (t, 4):
        raise ValueError("regions are one rectangle [4] or one per frame [%d, 4]; got %s" % (t, tuple(regions.shape)))
    x = frames.float()
    out = torch.empty((c, t, ho, wo), dtype=torch.float32, device=frames.device)
    for k, (top, left, h, w) in enumerate(regions.tolist()):
        out[:, k:k + 1] = torch.nn.functional.interpolate(x[:, k:k + 1, top:top + h, left:left + w], size=(ho, wo),
                                                          mode="bilinear", align_corners=False)
    return out


def box_regions(boxes, height: int, width: int, context: float = 1.0, square: bool = False, even: bool = False) -> torch.Tensor:
    """Float (x1, y1, x2, y2) boxes [..., 4] in the pixels of a height x width frame -> int64 (top, left, h, w) rectangles
    [..., 4] for `resized_crop` / `device_resized_crop` / `DevicePacker.video_batch(regions=)`.  The rule, in float64:
      1. the box is enlarged about its centre by `context` (a negative extent counts as 0);
      2. `square`: the shorter side is set to the longer one, about the same centre;
      3. the corners are clipped to [0, width] x [0, height];
      4. left = floor(x1), right = ceil(x2), top = floor(y1), bottom = ceil(y2): every pixel the box touches;
      5. at least one pixel: left <= width - 1, right >= left + 1 (a degenerate box, or one wholly outside the frame, becomes
         the pixel nearest to it); rows likewise;
      6. `even` (YUV 4:2:0 sources; `height` and `width` must be even): left and top go DOWN to even, right and bottom UP to
         even -- outward, still inside the frame --, so the rectangle is at least 2 x 2.  `even="width"` (YUV 4:2:2 sources;
         `width` must be even): left and right only.
    Boxes must be finite."""
    b = torch.as_tensor(boxes).detach().to("cpu", torch.float64)
    if b.dim() < 1 or b.shape[-1] != 4:
        raise ValueError("boxes are (x1, y1, x2, y2) [..., 4]; got %s" % (tuple(b.shape),))
    if not bool(torch.isfinite(b).all()):
        raise ValueError("boxes must be finite")
    height, width = int(height), int(width)
    if height < 1 or width < 1 or not context > 0:
        raise ValueError("height and width are positive ints and context a positive factor")
    if even == "width":
        if width % 2:
            raise ValueError("even='width' is for YUV 4:2:2 frames, whose width is even; got %d x %d" % (height, width))
    elif even and (height % 2 or width % 2):
        raise ValueError("even=True is for YUV 4:2:0 frames, whose height and width are even; got %d x %d" % (height, width))
    cx, cy = (b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2
    bw = torch.clamp(b[..., 2] - b[..., 0], min=0.0) * float(context)
    bh = torch.clamp(b[..., 3] - b[..., 1], min=0.0) * float(context)
    if square:
        bw = bh = torch.maximum(bw, bh)
    x1, x2 = torch.clamp(cx - bw / 2, 0.0, float(width)), torch.clamp(cx + bw / 2, 0.0, float(width))
    y1, y2 = torch.clamp(cy - bh / 2, 0.0, float(height)), torch.clamp(cy + bh / 2, 0.0, float(height))
    left = torch.clamp(torch.floor(x1).to(torch.int64), max=width - 1)
    top = torch.clamp(torch.floor(y1).to(torch.int64), max=height - 1)
    right = torch.maximum(torch.ceil(x2).to(torch.int64), left + 1)
    bottom = torch.maximum(torch.ceil(y2).to(torch.int64), top + 1)
    if even:
        left, right = left - left % 2, right + right % 2
    if even and even != "width":
        top, bottom = top - top % 2, bottom + bottom % 2
    return torch.stack([top, left, bottom - top, right - left], dim=-1)


def track_boxes_at(track_frames, track_boxes, frames) -> torch.Tensor:
    """A box track -- `track_boxes` [m, 4] at the strictly increasing frame numbers `track_frames` [m] -- evaluated at the
    frame numbers `frames` [n]: linear interpolation between the two neighbouring track points, the first / last box held
    outside the track.  Returns float64 [n, 4]."""
    tf = torch.as_tensor(track_frames).detach().to("cpu", torch.float64).reshape(-1)
    tb = torch.as_tensor(track_boxes).detach().to("cpu", torch.float64)
    at = torch.as_tensor(frames).detach().to("cpu", torch.float64).reshape(-1)
    if tf.numel() == 0 or tuple(tb.shape) != (tf.numel(), 4):
        raise ValueError("a track is frame numbers [m] and boxes [m, 4], m >= 1; got %s and %s" % (tuple(tf.shape), tuple(tb.shape)))
    if tf.numel() > 1 and not bool((tf[1:] > tf[:-1]).all()):
        raise ValueError("the frame numbers of a track increase strictly")
    hi = torch.clamp(torch.searchsorted(tf, at, right=True), max=tf.numel() - 1)
    lo = torch.clamp(hi - 1, min=0)
    span = tf[hi] - tf[lo]
    w = torch.where(span > 0, (at - tf[lo]) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(span))
    w = torch.clamp(w, 0.0, 1.0).unsqueeze(-1)
    return tb[lo] + w * (tb[hi] - tb[lo])


class ShortSideScale(torch.nn.Module):
    """transforms/transforms.py:100-121."""

    def __init__(self, size: int, interpolation: str = "bilinear", backend: str = "pytorch"):
        super().__init__()
        self._size, self._interpolation, self._backend = size, interpolation, backend

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return short_side_scale(x, self._size, self._interpolation, self._backend)


class UniformCropVideo(torch.nn.Module):
    """transforms/transforms.py:153-175: uniform_crop of x[video_key] with the spatial index x[aug_index_key]."""

    def __init__(self, size: int, video_key: str = "video", aug_index_key: str = "aug_index"):
        super().__init__()
        self._size, self._video_key, self._aug_index_key = size, video_key, aug_index_key

    def __call__(self, x: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x[self._video_key] = uniform_crop(x[self._video_key], self._size, x[self._aug_index_key])
        return x


# --------------------------------------------------------------------------- packed pixels (BGR24, 32-bit RGBA and kin)
# What an OpenCV pipeline holds ("BGR") and what screen capture, colour converters and compositor surfaces hand out (four
# bytes per pixel, the fourth unused, usually pitched): read where they lie by pv_batch_views / pv_frame_views /
# pv_region_views / pv_area_views (include/pv_mi355x.h, "packed pixels").  layout -> the bytes of R, G, B inside a pixel.
_PACKED_RGB = {"BGR": (2, 1, 0), "RGBA": (0, 1, 2), "BGRA": (2, 1, 0), "ARGB": (1, 2, 3), "ABGR": (3, 2, 1)}
PACKED_LAYOUTS = tuple(_PACKED_RGB)
_PACKED_ALIASES = {"RGBX": "RGBA", "BGRX": "BGRA", "XRGB": "ARGB", "XBGR": "ABGR"}     # the fourth byte is unused either way
_PACKED_ANY = PACKED_LAYOUTS + tuple(_PACKED_ALIASES)


def _packed_name(layout):
    """The layout of `PACKED_LAYOUTS` behind a packed `src_layout` string (an "X" spelling is its "A" one), else None."""
    layout = _PACKED_ALIASES.get(layout, layout) if isinstance(layout, str) else None
    return layout if layout in _PACKED_RGB else None


def _packed_bytes(layout):
    """Bytes per pixel of a packed layout: 3 for "BGR", 4 for the others."""
    return 3 if _packed_name(layout) == "BGR" else 4


def packed_to_rgb(x: torch.Tensor, layout: str) -> torch.Tensor:
    """The host mirror of the packed layouts: [..., PB] pixels in `layout` -> [..., 3] in R, G, B order, by a pure index (no
    arithmetic; the fourth byte of a 32-bit pixel is dropped).  The ingest holds, bit for bit, what it writes for
    `packed_to_rgb(video, layout).contiguous()` read as "NTHWC"."""
    name = _packed_name(layout)
    if name is None:
        raise ValueError("a packed layout is one of %s, got %r" % (PACKED_LAYOUTS, layout))
    if x.shape[-1] != _packed_bytes(name):
        raise ValueError("%s pixels have %d bytes, the last dimension has %d" % (name, _packed_bytes(name), x.shape[-1]))
    return x[..., list(_PACKED_RGB[name])]


def packed_geometry(frames: torch.Tensor, layout: str) -> dict:
    """Where the pixels of packed frames lie: `frames` is uint8 [N, H, W, PB] (or [H, W, PB]: one frame) with
    stride(-1) == 1, stride(-2) == PB and a row stride >= W * PB -- a pitched surface, or a column slice of a wider one, is
    read where it lies; the frame stride may be anything that keeps the frames apart.  Returns N, Hs, Ws and the record's
    fields in BYTES: y_pitch (the row stride), frame_stride (between frames; one frame: its extent) and zero u_offset /
    v_offset / c_pitch.  ValueError, naming the stride, for anything else: no copy is ever made."""
    name = _packed_name(layout)
    if name is None:
        raise ValueError("a packed layout is one of %s, got %r" % (PACKED_LAYOUTS, layout))
    pb = _packed_bytes(name)
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[-1] != pb or frames.dtype != torch.uint8:
        raise ValueError("%s frames are uint8 [N, H, W, %d], got %s %s" % (name, pb, frames.dtype, tuple(frames.shape)))
    n, h, w, _ = frames.shape
    if frames.stride(3) != 1:
        raise ValueError("%s frames: stride(-1) is %d, not 1: the bytes of a pixel are adjacent" % (name, frames.stride(3)))
    if frames.stride(2) != pb:
        raise ValueError("%s frames: stride(-2) is %d, not %d: the pixels of a row are adjacent" % (name, frames.stride(2), pb))
    pitch = frames.stride(1) if h > 1 else max(frames.stride(1), w * pb)
    if pitch < w * pb:
        raise ValueError("%s frames: the row stride, stride(-3), is %d, less than the %d bytes of a row" % (name, pitch, w * pb))
    extent = (h - 1) * pitch + w * pb
    frame_stride = frames.stride(0) if n > 1 else extent
    if frame_stride < extent:
        raise ValueError("%s frames: the frame stride, stride(0), is %d, less than the %d bytes of a frame" % (name, frame_stride, extent))
    if pb == 4 and (pitch % 4 or frame_stride % 4 or frames.data_ptr() % 4):
        raise ValueError("%s frames: a 4-byte pixel is one aligned dword -- the address, the row stride %d and the frame stride %d "
                         "are multiples of 4" % (name, pitch, frame_stride))
    return dict(N=n, Hs=h, Ws=w, y_pitch=pitch, frame_stride=frame_stride, u_offset=0, v_offset=0, c_pitch=0)


# --------------------------------------------------------------------------- YUV 4:2:0 sources
YUV_LAYOUTS = ("NV12", "NV21", "I420", "YV12")
# 16-bit little-endian samples.  P0xx: the NV12 arrangement with the value in the HIGH bits (what a hardware decoder writes for
# 10- / 12- / 16-bit streams); I0xx: the I420 arrangement with the value in the LOW bits (yuv420p10le and friends).
YUV16_LAYOUTS = ("P010", "P012", "P016", "I010", "I012", "I016")
# YUV 4:2:2 and 4:4:4 (include/pv_mi355x.h, "YUV 4:2:2 and 4:4:4"), read by the item-sourced entry points only.  I422 / YV16:
# yuv422p / yuvj422p (MJPEG cameras), U (V) first; NV16 / NV61: one interleaved chroma plane, U (V) first; P210 / P212 / P216:
# NV16's arrangement with 16-bit samples, the value in the HIGH bits; I210 / I212 / I216: yuv422p10le and kin, the value in the
# LOW bits.  I444 / YV24: yuv444p / yuvj444p; I410 / I412 / I416: yuv444p10le and kin.  (NV24 / NV42 have no string: the C ABI
# reads them -- PV_SRC_YUV444 with c_step 2.)
YUV422_LAYOUTS = ("I422", "YV16", "NV16", "NV61", "P210", "P212", "P216", "I210", "I212", "I216")
YUV444_LAYOUTS = ("I444", "YV24", "I410", "I412", "I416")
# Packed YUV 4:2:2 (include/pv_mi355x.h, "packed YUV 4:2:2"), read by the item-sourced entry points only: ONE plane of
# macropixels of four samples, frames [N, H, W, 2] (`yuyv_geometry`).  YUY2 ("YUYV" is an alias): Y0 U Y1 V, what UVC webcams
# and V4L2 hand out; YVYU: Y0 V Y1 U; UYVY: U Y0 V Y1, what SDI / HDMI capture cards hand out; Y210 / Y212 / Y216: YUY2's
# order with 16-bit samples, the value in the HIGH bits.  (VYUY has no string: the C ABI reads it.)
YUYV_LAYOUTS = ("YUY2", "YVYU", "UYVY", "Y210", "Y212", "Y216")
_YUYV_ALIASES = {"YUYV": "YUY2"}
_YUYV_ANY = YUYV_LAYOUTS + tuple(_YUYV_ALIASES)
_YUYV_UV = {"YUY2": (1, 3), "YVYU": (3, 1), "UYVY": (0, 2), "Y210": (1, 3), "Y212": (1, 3), "Y216": (1, 3)}   # the samples of U, V
_YUV4_ANY = YUV422_LAYOUTS + YUV444_LAYOUTS + _YUYV_ANY    # the YUV layouts of the item-sourced entry points only
_YUV_ANY = YUV_LAYOUTS + YUV16_LAYOUTS + _YUV4_ANY
_YUV_INTERLEAVED = ("NV12", "NV21", "P010", "P012", "P016", "NV16", "NV61", "P210", "P212", "P216")
_YUV_V_FIRST = ("NV21", "YV12", "YV16", "NV61", "YV24")
_YUV_PLANE_FIELDS = ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch")   # of `yuv_geometry`, a descriptor, a record
_SRC_LAYOUTS = ("NCTHW", "NTHWC") + _YUV_ANY + _PACKED_ANY      # every `src_layout` the device ingest takes
_LAYOUT_ERROR = ("src_layout is 'NCTHW', 'NTHWC' or one of %s" % (YUV_LAYOUTS,) + " or %s" % (YUV16_LAYOUTS,)
                 + " or %s" % (YUV422_LAYOUTS,) + " or %s" % (YUV444_LAYOUTS,) + " or %s" % (PACKED_LAYOUTS,)
                 + " or %s" % (YUYV_LAYOUTS,))
_YUV16_DEPTH = {"P010": (10, True), "P012": (12, True), "P016": (16, True), "I010": (10, False), "I012": (12, False),
                "I016": (16, False),                       # layout -> (bit depth, MSB-aligned)
                "P210": (10, True), "P212": (12, True), "P216": (16, True), "I210": (10, False), "I212": (12, False),
                "I216": (16, False), "I410": (10, False), "I412": (12, False), "I416": (16, False),
                "Y210": (10, True), "Y212": (12, True), "Y216": (16, True)}
_YUV_WIDE = tuple(_YUV16_DEPTH)                            # every layout of 16-bit samples (PV_U16)


def _yuyv_name(layout):
    """The layout of `YUYV_LAYOUTS` behind a packed 4:2:2 `src_layout` string ("YUYV" is "YUY2"), else None."""
    layout = _YUYV_ALIASES.get(layout, layout) if isinstance(layout, str) else None
    return layout if layout in YUYV_LAYOUTS else None


def _yuv_sub(layout):
    """(csy, csx) of a YUV layout: the chroma sample of luma pixel (y, x) is (y >> csy, x >> csx)."""
    return (0, 1) if layout in YUV422_LAYOUTS or layout in _YUYV_ANY else (0, 0) if layout in YUV444_LAYOUTS else (1, 1)


def _yuv_c_step(layout):
    """`c_step` of a YUV layout: the samples between x-adjacent samples of one chroma component."""
    return 4 if layout in _YUYV_ANY else 2 if layout in _YUV_INTERLEAVED else 1


def _yuv_dims(layout):
    """The dimensions of ONE FRAME of a YUV layout: 2 ([rows, W]), or 3 for packed 4:2:2 ([H, W, 2])."""
    return 3 if layout in _YUYV_ANY else 2


def region_evenness(src_layout):
    """The `even` of `box_regions` / of the rectangle check for a source layout: True (YUV 4:2:0: all four members even),
    "width" (YUV 4:2:2, planar or packed: left and w) or False (everything else, YUV 4:4:4 included)."""
    if src_layout not in _YUV_ANY or src_layout in YUV444_LAYOUTS:
        return False
    return "width" if src_layout in YUV422_LAYOUTS or src_layout in _YUYV_ANY else True
_YUV_KR_KB = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
_YUV_KR_KB_DEEP = {"bt2020": (0.2627, 0.0593)}             # Rec. 2020 defines 10- and 12-bit quantisation only: no 8-bit form


def yuv_matrix(standard: str = "bt709", full_range: bool = False, bit_depth: int = 8, msb_aligned: bool = False) -> torch.Tensor:
    """The 3 x 4 fp64 matrix M with (R, G, B) = M . (Y, U, V, 1) for 8-bit Y'CbCr, RGB in [0, 255]: rows R, G, B, columns
    Y, U, V and a constant.  Derived from the standard's luma coefficients (Kr, Kb) -- Y' = Kr R' + Kg G' + Kb B',
    Pb = (B' - Y') / (2 (1 - Kb)), Pr = (R' - Y') / (2 (1 - Kr)) -- and the quantisation: limited range puts Y' in 16..235
    and Pb, Pr in 16..240 around 128, full range in 0..255 around 128.

    `bit_depth` d in 8..16 (RGB stays in [0, 255]): limited range puts Y' in 16 * 2^(d-8) .. 235 * 2^(d-8) and gives Pb, Pr a
    span of 224 * 2^(d-8); full range is 0 .. 2^d - 1; the chroma centre is 2^(d-1) for both.  `msb_aligned`: the value sits in
    the high bits of a 16-bit code (P010 / P012 / P016), so the Y, U, V columns are scaled by 2^-(16-d) -- exactly.  The ingest
    applies no shift and no mask of its own: depth and alignment live here.  The defaults give the 8-bit matrix bit for bit.
    "bt2020" (Kr 0.2627, Kb 0.0593; what 10-bit streams usually signal) takes a `bit_depth` of 10 or more: the standard
    defines no 8-bit quantisation."""
    deep = standard in _YUV_KR_KB_DEEP
    if standard not in _YUV_KR_KB and not (deep and isinstance(bit_depth, int) and bit_depth >= 10):
        raise ValueError("standard is one of %s, got %r" % (sorted(_YUV_KR_KB), standard)
                         + (" (bt2020 takes bit_depth >= 10, got %r)" % (bit_depth,) if deep else ""))
    if not isinstance(bit_depth, int) or not 8 <= bit_depth <= 16:
        raise ValueError("bit_depth is an integer in 8..16, got %r" % (bit_depth,))
    kr, kb = _YUV_KR_KB_DEEP[standard] if deep else _YUV_KR_KB[standard]
    kg = 1.0 - kr - kb
    k = float(1 << (bit_depth - 8))                        # codes per 8-bit code: a power of two, so the products with it are exact
    top = float((1 << bit_depth) - 1)
    y_lo, y_span, c_span = (0.0, top, top) if full_range else (16.0 * k, 219.0 * k, 224.0 * k)
    ys, cs = 255.0 / y_span, 255.0 / c_span
    m = torch.tensor([[ys, 0.0, 2.0 * (1.0 - kr) * cs],
                      [ys, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs],
                      [ys, 2.0 * (1.0 - kb) * cs, 0.0]], dtype=torch.float64)
    const = -(m[:, 0] * y_lo + (m[:, 1] + m[:, 2]) * (128.0 * k))
    if msb_aligned:
        m = m * (1.0 / float(1 << (16 - bit_depth)))
    return torch.cat([m, const[:, None]], dim=1)


def _yuv_matrix_of(yuv, layout=None) -> torch.Tensor:
    """`yuv` as every YUV entry point takes it: (standard, full_range) -- composed with the depth and the bit alignment of a
    16-bit `layout` --, or an explicit 3 x 4 matrix, taken as it is."""
    if isinstance(yuv, (tuple, list)) and len(yuv) == 2 and isinstance(yuv[0], str):
        depth, msb = _YUV16_DEPTH.get(layout, (8, False))
        return yuv_matrix(yuv[0], bool(yuv[1]), depth, msb)
    m = torch.as_tensor(yuv, dtype=torch.float64).cpu()
    if tuple(m.shape) != (3, 4):
        raise ValueError("yuv is (standard, full_range) or a 3 x 4 matrix, got shape %s" % (tuple(m.shape),))
    return m


def yuyv_geometry(frames: torch.Tensor, layout: str) -> dict:
    """Where the samples of packed YUV 4:2:2 frames lie (`YUYV_LAYOUTS`; "YUYV" is "YUY2"): `frames` is [N, H, W, 2] (or
    [H, W, 2]: one frame; what `cv2.VideoCapture` hands out with CAP_PROP_CONVERT_RGB = 0) -- uint8, or uint16 / int16 for Y210 /
    Y212 / Y216 -- with an even W, stride(-1) == 1, stride(-2) == 2 and a row stride >= 2 * W, counted in ELEMENTS: a pitched
    surface, or a column slice of a wider one that starts at an even column, is read where it lies; the frame stride may be
    anything that keeps the frames apart.  Returns N, Hs, Ws, the subsampling (csy, csx) = (0, 1), c_step 4 and the record's
    fields in BYTES: y_pitch (the row stride), frame_stride (between frames; one frame: its extent), c_pitch 0 and u_offset /
    v_offset, the byte of the first U / V sample from the start of a row.  ValueError, naming the stride, for anything else: no
    copy is ever made."""
    name = _yuyv_name(layout)
    if name is None:
        raise ValueError("a packed YUV 4:2:2 layout is one of %s, got %r" % (YUYV_LAYOUTS, layout))
    wide = name in _YUV_WIDE
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[-1] != 2 or (frames.dtype not in (torch.uint16, torch.int16) if wide else frames.dtype != torch.uint8):
        raise ValueError("%s frames are %s [N, H, W, 2], got %s %s" % (name, "uint16 or int16" if wide else "uint8", frames.dtype, tuple(frames.shape)))
    n, h, w, _ = frames.shape
    if n == 0 or h == 0 or w == 0 or w % 2:
        raise ValueError("%s frames: a row is W / 2 macropixels of two pixels, W is even and positive; got %d frames of %d x %d" % (name, n, h, w))
    if frames.stride(3) != 1:
        raise ValueError("%s frames: stride(-1) is %d, not 1: the two samples of a pixel are adjacent" % (name, frames.stride(3)))
    if frames.stride(2) != 2:
        raise ValueError("%s frames: stride(-2) is %d, not 2: the pixels of a row are adjacent" % (name, frames.stride(2)))
    pitch = frames.stride(1) if h > 1 else max(frames.stride(1), 2 * w)
    if pitch < 2 * w:
        raise ValueError("%s frames: the row stride, stride(-3), is %d, less than the %d samples of a row" % (name, pitch, 2 * w))
    extent = (h - 1) * pitch + 2 * w
    frame_stride = frames.stride(0) if n > 1 else extent
    if frame_stride < extent:
        raise ValueError("%s frames: the frame stride, stride(0), is %d, less than the %d samples of a frame" % (name, frame_stride, extent))
    sb = 2 if wide else 1                                   # elements -> bytes
    u, v = _YUYV_UV[name]
    return dict(N=n, Hs=h, Ws=w, Hc=h, frame_stride=frame_stride * sb, y_pitch=pitch * sb, c_pitch=0, c_step=4,
                u_offset=u * sb, v_offset=v * sb, csy=0, csx=1)


def yuyv_to_planar(frames: torch.Tensor, layout: str) -> torch.Tensor:
    """The host mirror of the packed 4:2:2 layouts, by a pure index (no arithmetic): [N, H, W, 2] (or [H, W, 2]) frames in
    `layout` -> the contiguous I422-arranged copy [N, 2H, W] (or [2H, W]) of the same dtype -- H rows of luma, then H rows of U
    and H rows of V at half the pitch, which is "I422" for uint8 and "I216" for 16-bit samples (the codes are not touched, so
    the matrix of the packed layout goes with it).  The ingest holds, bit for bit, what it writes for that copy."""
    name = _yuyv_name(layout)
    if name is None:
        raise ValueError("a packed YUV 4:2:2 layout is one of %s, got %r" % (YUYV_LAYOUTS, layout))
    g = yuyv_geometry(frames, name)
    one = frames.dim() == 3
    x = frames[None] if one else frames
    if frames.dtype == torch.uint16:
        x = x.view(torch.int16)                             # the same bits, in the type every operator has
    h, w = g["Hs"], g["Ws"]
    u, v = _YUYV_UV[name]
    flat = x.reshape(x.shape[0], h, w // 2, 4)             # a row as macropixels of four samples
    luma = flat[..., [1 - (u & 1), 3 - (u & 1)]].reshape(-1, h, w)
    chroma = [flat[..., k].reshape(-1, h * (w // 2)) for k in (u, v)]                        # H rows of W / 2 samples each
    planar = torch.cat([luma.reshape(-1, h * w)] + chroma, dim=1).reshape(-1, 2 * h, w).view(frames.dtype)
    return planar[0] if one else planar


def yuv_geometry(frames: torch.Tensor, layout: str, coded_height=None, height=None) -> dict:
    """Where the samples of YUV frames are, in bytes, read off the tensor's shape and strides (nothing is copied).

    4:2:0 (`YUV_LAYOUTS`, `YUV16_LAYOUTS`): `frames` is uint8 [N, Hc*3/2, W] (a video) or [B, T', Hc*3/2, W] (clips; then
    N = B * T' and clip b starts at frame b * T'), Hc being the coded height: Hc luma rows, then the chroma.  `height` is the
    display height Hs <= Hc (default Hc) and `coded_height`, when given, is checked against the shape.  The only stride
    requirement is stride(-1) == 1: the row pitch P = stride(-2) may exceed W and the frame stride the frame, so a pitched
    decoder surface is read in place.  NV12 / NV21: chroma row j is tensor row Hc + j, U and V (V and U) interleaved.
    I420 / YV12: two planes of Hc/2 rows with pitch P/2 behind the luma, U (V) first -- for P == W exactly the contiguous
    yuv420p frame.

    4:2:2 (`YUV422_LAYOUTS`): [N, Hc*2, W] with the same stride rules, W even, any Hc and Hs.  I422 / YV16 and their 16-bit
    kin: two planes of Hc rows with pitch P/2 behind the luma, U (V) first -- for P == W exactly the contiguous yuv422p frame.
    NV16 / NV61 / P21x: Hc rows of interleaved U and V (V and U) at pitch P.
    4:4:4 (`YUV444_LAYOUTS`): [N, Hc*3, W], any W, Hc and Hs: three planes of Hc rows at pitch P, Y, U, V (YV24: Y, V, U).
    For these two the result also carries the subsampling, csy and csx: the chroma of pixel (y, x) is (y >> csy, x >> csx).

    The layouts of 16-bit samples -- `YUV16_LAYOUTS` (P010 / P012 / P016: NV12's arrangement; I010 / I012 / I016: I420's,
    yuv420p10le), P210 / I210 / I410 and their 12- and 16-bit kin -- take torch.uint16 or torch.int16 (the same bits; decoder
    bindings differ) with the same shape and stride rules IN ELEMENTS, and the returned frame_stride, pitches and offsets are
    BYTES, as the descriptors take them (c_step stays 2 / 1: samples).

    Packed 4:2:2 (`YUYV_LAYOUTS`): frames [N, H, W, 2], [B, T, H, W, 2] or [H, W, 2] -- `yuyv_geometry`, whose result this is
    (c_step 4); there is no coded height beside the shape's, so `coded_height` and `height`, when given, are H."""
    if layout in _YUYV_ANY:
        lead = tuple(frames.shape[:2]) if frames.dim() == 5 else None
        if lead is not None:                                # clips: one sequence of B * T frames, as below
            if lead[0] > 1 and lead[1] > 1 and frames.stride(0) != lead[1] * frames.stride(1):
                raise RuntimeError("clips [B, T, ...] are one sequence of B * T frames: stride(0) == T * stride(1); got %s" % (frames.stride(),))
            seq = frames[0] if lead[0] == 1 else frames[:, 0] if lead[1] == 1 else frames.as_strided(
                (lead[0] * lead[1],) + tuple(frames.shape[2:]), frames.stride()[1:])
            g = yuyv_geometry(seq, layout)
        else:
            g = yuyv_geometry(frames, layout)
        for what, given in (("coded_height", coded_height), ("height", height)):
            if given is not None and int(given) != g["Hs"]:
                raise RuntimeError("%s %d, but %s frames have the %d rows of their shape" % (what, given, layout, g["Hs"]))
        return g
    if layout not in _YUV_ANY:
        raise ValueError("a YUV layout is one of %s, got %r" % (YUV_LAYOUTS, layout) + " (16-bit samples: %s;" % (YUV16_LAYOUTS,)
                         + " 4:2:2: %s; 4:4:4: %s; packed 4:2:2: %s)" % (YUV422_LAYOUTS, YUV444_LAYOUTS, YUYV_LAYOUTS))
    wide = layout in _YUV_WIDE
    csy, csx = _yuv_sub(layout)
    num, den = {(1, 1): (3, 2), (0, 1): (2, 1), (0, 0): (3, 1)}[(csy, csx)]     # tensor rows per coded luma row
    form = "Hc*3/2" if csy else "Hc*%d" % num
    if frames.dim() not in (3, 4) or (frames.dtype not in (torch.uint16, torch.int16) if wide else frames.dtype != torch.uint8):
        raise RuntimeError("%s frames are %s [N, %s, W] or [B, T, %s, W], got %s %s"
                           % (layout, "uint16 or int16" if wide else "uint8", form, form, frames.dtype, tuple(frames.shape)))
    rows, w = frames.shape[-2:]
    hc = rows * den // num
    if csy:
        if rows == 0 or hc * 3 != rows * 2 or hc % 2 or w % 2 or w == 0:
            raise RuntimeError("%d x %d is not Hc*3/2 rows of an even width W with an even coded height Hc" % (rows, w))
    elif rows == 0 or hc * num != rows or w == 0 or (csx and w % 2):
        raise RuntimeError("%d x %d is not %s rows of %s width W" % (rows, w, form, "an even" if csx else "a"))
    if coded_height is not None and coded_height != hc:
        raise RuntimeError("coded_height %d, but the frames have %d = %d * %d / %d rows" % (coded_height, rows, hc, num, den))
    hs = hc if height is None else int(height)
    if not 0 < hs <= hc or (csy and hs % 2):
        raise RuntimeError("the display height %d is %sat most the coded height %d" % (hs, "even and " if csy else "", hc))
    pitch = frames.stride(-2)
    if frames.stride(-1) != 1 or pitch < w:
        raise RuntimeError("%s frames have stride(-1) == 1 and a row pitch >= W; got strides %s" % (layout, frames.stride()))
    if frames.dim() == 4 and frames.shape[0] > 1 and frames.shape[1] > 1 and frames.stride(0) != frames.shape[1] * frames.stride(1):
        raise RuntimeError("clips [B, T, ...] are one sequence of B * T frames: stride(0) == T * stride(1); got %s" % (frames.stride(),))
    n = frames.shape[0] if frames.dim() == 3 else frames.shape[0] * frames.shape[1]
    frame_stride = frames.stride(-3) if frames.shape[-3] > 1 else (frames.stride(0) if frames.dim() == 4 and frames.shape[0] > 1 else rows * pitch)
    if frame_stride < (rows - 1) * pitch + w:
        raise RuntimeError("frames overlap: frame stride %d for %d rows of pitch %d" % (frame_stride, rows, pitch))
    first = hc * pitch
    swap = layout in _YUV_V_FIRST
    if layout in _YUV_INTERLEAVED:
        c_step, c_pitch = 2, pitch
        u, v = (first + 1, first) if swap else (first, first + 1)
    else:
        if csx and pitch % 2:
            raise RuntimeError("%s chroma rows have half the luma pitch: the pitch %d must be even" % (layout, pitch))
        c_step, c_pitch = 1, pitch >> csx
        second = first + (hc >> csy) * c_pitch
        u, v = (second, first) if swap else (first, second)
    sb = 2 if wide else 1                                   # elements -> bytes
    g = dict(N=n, Hs=hs, Ws=w, Hc=hc, frame_stride=frame_stride * sb, y_pitch=pitch * sb, c_pitch=c_pitch * sb, c_step=c_step,
             u_offset=u * sb, v_offset=v * sb)
    if layout in _YUV4_ANY:
        g.update(csy=csy, csx=csx)
    return g


def yuv_to_rgb(frames: torch.Tensor, layout: str, matrix, coded_height=None, height=None) -> torch.Tensor:
    """The virtual RGB frame the YUV ingest takes its taps from (include/pv_mi355x.h), on the host, for EVERY YUV layout: fp32
    [..., 3, Hs, Ws] with rgb(y, x) = clamp(M . (Y[y][x], U[y >> csy][x >> csx], V[y >> csy][x >> csx], 1), 0, 255), NOT
    rounded to an integer -- chroma is replicated over the luma pixels it covers: 2 x 2 for 4:2:0, 1 x 2 for 4:2:2, none
    for 4:4:4.  `frames`, `layout`, `coded_height` and `height` as in `yuv_geometry`; `matrix` is a 3 x 4 matrix
    (`yuv_matrix`).  The conversion runs in fp64 and is rounded once to fp32.  16-bit codes are read UNSIGNED, whichever of
    uint16 / int16 the tensor is.  A layout of `YUYV_LAYOUTS` (frames [..., H, W, 2]) gives what its `yuyv_to_planar` copy gives."""
    if layout in _YUYV_ANY:
        frames = frames.cpu() if frames.is_cuda else frames
        lead = tuple(frames.shape[:-3])
        planar = yuyv_to_planar(frames.reshape((-1,) + tuple(frames.shape[-3:])), layout)
        rgb = yuv_to_rgb(planar, "I216" if layout in _YUV_WIDE else "I422", matrix, coded_height, height)
        return rgb.reshape(lead + tuple(rgb.shape[-3:]))
    g = yuv_geometry(frames, layout, coded_height, height)
    m = torch.as_tensor(matrix, dtype=torch.float64).cpu()
    if tuple(m.shape) != (3, 4):
        raise ValueError("matrix is 3 x 4, got %s" % (tuple(m.shape),))
    frames = frames.cpu() if frames.is_cuda else frames
    sb = 2 if layout in _YUV_WIDE else 1                    # the geometry is bytes, as_strided counts elements
    if frames.dtype == torch.uint16:
        frames = frames.view(torch.int16)                   # the same bits, in the type every CPU operator has
    lead, lead_strides = tuple(frames.shape[:-2]), tuple(frames.stride()[:-2])
    off = frames.storage_offset()
    csy, csx = g.get("csy", 1), g.get("csx", 1)

    def plane(rows, cols, pitch, step, start):
        p = torch.as_strided(frames, lead + (rows, cols), lead_strides + (pitch // sb, step), off + start // sb).to(torch.float64)
        return torch.where(p < 0, p + 65536.0, p) if sb == 2 else p

    y = plane(g["Hs"], g["Ws"], g["y_pitch"], 1, 0)
    hcr, wcr = (g["Hs"] + csy) >> csy, (g["Ws"] + csx) >> csx
    u = plane(hcr, wcr, g["c_pitch"], g["c_step"], g["u_offset"])
    v = plane(hcr, wcr, g["c_pitch"], g["c_step"], g["v_offset"])
    if csy:
        u, v = [c.repeat_interleave(2, -2) for c in (u, v)]
    if csx:
        u, v = [c.repeat_interleave(2, -1) for c in (u, v)]
    yuv1 = torch.stack([y, u, v, torch.ones_like(y)], dim=-3)                       # [..., 4, Hs, Ws]
    rgb = torch.einsum("ck,...khw->...chw", m, yuv1)
    return torch.clamp(rgb, 0.0, 255.0).float()


def yuv420_to_rgb(frames: torch.Tensor, layout: str, matrix, coded_height=None, height=None) -> torch.Tensor:
    """The virtual RGB frame `pv_yuv_views` takes its taps from (include/pv_mi355x.h), on the host: fp32 [..., 3, Hs, Ws] with
    rgb(y, x) = clamp(M . (Y[y][x], U[y >> 1][x >> 1], V[y >> 1][x >> 1], 1), 0, 255), NOT rounded to an integer.  Chroma is
    replicated over its 2 x 2 luma block.  `frames`, `layout`, `coded_height` and `height` as in `yuv_geometry`; `matrix`
    is a 3 x 4 matrix (`yuv_matrix`).  The conversion runs in fp64 and is rounded once to fp32.  The 16-bit codes of a
    `YUV16_LAYOUTS` layout are read UNSIGNED, whichever of uint16 / int16 the tensor is (`pv_yuv16_views`).  `yuv_to_rgb` with
    a 4:2:0 layout: the name the 4:2:0 paths have always called."""
    if layout not in YUV_LAYOUTS + YUV16_LAYOUTS:
        raise ValueError("a YUV 4:2:0 layout is one of %s, got %r" % (YUV_LAYOUTS, layout) + " (16-bit samples: %s)" % (YUV16_LAYOUTS,))
    return yuv_to_rgb(frames, layout, matrix, coded_height, height)


# --------------------------------------------------------------------------- HDR sources: PQ / HLG taps to BT.709 SDR
HDR_TRANSFERS = ("pq", "hlg")
HDR_GAMUTS = {"bt2020_to_bt709": ((1.6605, -0.5876, -0.0728), (-0.1246, 1.1329, -0.0083), (-0.0182, -0.1006, 1.1187)),   # BT.2087
              None: ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))}
_PQ_M1, _PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
_PQ_C1, _PQ_C2, _PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
_HLG_A = 0.17883277
_HLG_B = 1.0 - 4.0 * _HLG_A
_HLG_C = 0.5 - _HLG_A * math.log(4.0 * _HLG_A)
_OETF_BETA, _OETF_ALPHA = 0.018053968510807, 1.09929682680944          # BT.2020's continuous constants
_TONE_OFF = 3e38                                                        # a knee no light reaches: the curve is never taken


def tone_params(transfer: str, peak_nits: float = 1000.0, white_nits: float = 203.0, knee: float = 0.3, tone_map: str = "mobius",
                gamut="bt2020_to_bt709") -> torch.Tensor:
    """The fp32 [16] `tone` table of `pv_hdr_views` (include/pv_mi355x.h, "HDR sources"), composed in float64:
    [0] the scale to SDR reference white (PQ: 10000 / white_nits; HLG: peak_nits / white_nits), [1] HLG's system gamma - 1
    (gamma = 1.2 + 0.42 log10(peak_nits / 1000); 0 for PQ), [2..5] the knee j and s, a', b' of the hue-preserving "mobius"
    curve on max-RGB -- the identity up to j, C1 there, and P = peak_nits / white_nits goes to 1 -- or, `tone_map="clip"`,
    a knee that is never reached, [6..14] the gamut matrix row-major (`gamut=None`: the identity), [15] 0."""
    if transfer not in HDR_TRANSFERS:
        raise ValueError("transfer is one of %s, got %r" % (HDR_TRANSFERS, transfer))
    if tone_map not in ("mobius", "clip"):
        raise ValueError("tone_map is 'mobius' or 'clip', got %r" % (tone_map,))
    if gamut not in HDR_GAMUTS:
        raise ValueError("gamut is 'bt2020_to_bt709' or None, got %r" % (gamut,))
    peak, white, j = float(peak_nits), float(white_nits), float(knee)
    if not (white > 0.0 and peak > white):
        raise ValueError("peak_nits lies above white_nits, and both are positive: got %r and %r" % (peak_nits, white_nits))
    if not 0.0 < j < 1.0:
        raise ValueError("knee lies inside (0, 1), got %r" % (knee,))
    p = peak / white
    if transfer == "pq":
        head = [10000.0 / white, 0.0]
    else:
        head = [p, 1.2 + 0.42 * math.log10(peak / 1000.0) - 1.0]
    if tone_map == "clip":
        curve = [_TONE_OFF, 1.0, 0.0, 0.0]
    else:
        a = -j * j * (p - 1.0) / (j * j - 2.0 * j + p)
        b = (j * j - 2.0 * j * p + p) / (p - 1.0)
        curve = [j, (b * b + 2.0 * b * j + j * j) / (b - a), a, b]
    return torch.tensor(head + curve + [g for row in HDR_GAMUTS[gamut] for g in row] + [0.0], dtype=torch.float64).float()


def _transfer_code(transfer):
    if isinstance(transfer, str) and transfer in HDR_TRANSFERS:
        return HDR_TRANSFERS.index(transfer) + 1               # PV_TRANSFER_PQ = 1, PV_TRANSFER_HLG = 2
    if transfer in (1, 2) and not isinstance(transfer, bool):
        return int(transfer)
    raise ValueError("transfer is one of %s, got %r" % (HDR_TRANSFERS, transfer))


def hdr_to_sdr(rgb255: torch.Tensor, transfer, tone) -> torch.Tensor:
    """The tap map of `pv_hdr_views` on the host, in float64: `rgb255` [..., 3, H, W] holds BT.2020 R'G'B' under the PQ or HLG
    curve in 0..255 -- what `yuv420_to_rgb` gives for an HDR stream's matrix --, `tone` is `tone_params`' table (its fp32
    values are what the device computes with).  Returns the BT.709-coded SDR frame in 0..255, float64, same shape: every
    pixel on its own, to linear light, the tone curve on max-RGB, the gamut matrix with its clamp, BT.2020's OETF."""
    code = _transfer_code(transfer)
    t = torch.as_tensor(tone).detach().to("cpu", torch.float64).reshape(-1)
    if t.numel() != 16:
        raise ValueError("tone holds 16 values (tone_params), got %d" % t.numel())
    x = torch.as_tensor(rgb255).detach().to("cpu", torch.float64)
    if x.dim() < 3 or x.shape[-3] != 3:
        raise ValueError("expected [..., 3, H, W], got %s" % (tuple(x.shape),))
    e = x / 255.0
    if code == 1:
        p = e ** (1.0 / _PQ_M2)
        lin = (torch.clamp(p - _PQ_C1, min=0.0) / (_PQ_C2 - _PQ_C3 * p)) ** (1.0 / _PQ_M1) * t[0]
    else:
        s = torch.where(e <= 0.5, e * e / 3.0, (torch.exp((e - _HLG_C) / _HLG_A) + _HLG_B) / 12.0)
        ys = 0.2627 * s[..., 0:1, :, :] + 0.6780 * s[..., 1:2, :, :] + 0.0593 * s[..., 2:3, :, :]
        gain = torch.where(ys > 0.0, torch.clamp(ys, min=1e-300) ** t[1] * t[0], torch.zeros_like(ys))
        lin = s * gain
    m = lin.amax(dim=-3, keepdim=True)
    safe = torch.where(m > t[2], m, torch.ones_like(m))
    lin = lin * torch.where(m > t[2], t[3] * (safe + t[4]) / ((safe + t[5]) * safe), torch.ones_like(m))
    lin = torch.clamp(torch.einsum("ck,...khw->...chw", t[6:15].reshape(3, 3), lin), 0.0, 1.0)
    v = torch.where(lin < _OETF_BETA, 4.5 * lin, _OETF_ALPHA * lin ** 0.45 - (_OETF_ALPHA - 1.0))
    return 255.0 * v


def _hdr_of(hdr, src_layout):
    """`hdr` as every entry point takes it -- None, "pq" / "hlg" (`tone_params` with its defaults) or (transfer, tone tensor)
    -- as (PV_TRANSFER code, fp32 [16] host tensor), or None.  ValueError for anything else, and for a source layout that is
    not one of `YUV16_LAYOUTS`: 8-bit and RGB HDR sources do not exist in practice, and no path may drop the map."""
    if hdr is None:
        return None
    if isinstance(hdr, str):
        hdr = (hdr, tone_params(hdr))
    if not (isinstance(hdr, (tuple, list)) and len(hdr) == 2 and isinstance(hdr[1], torch.Tensor)):
        raise ValueError("hdr is None, 'pq', 'hlg' or (transfer, tone_params(...)), got %r" % (hdr,))
    code = _transfer_code(hdr[0])
    tone = hdr[1].detach().to("cpu", torch.float32).reshape(-1).contiguous()
    if tone.numel() != 16:
        raise ValueError("tone holds 16 values (tone_params), got %d" % tone.numel())
    if src_layout not in YUV16_LAYOUTS:
        raise ValueError("hdr= maps the taps of a 10- to 16-bit YUV 4:2:0 source (src_layout one of %s), not of %r%s"
                         % (YUV16_LAYOUTS, src_layout,
                            ": pv_hdr_views does not read packed YUV 4:2:2" if src_layout in _YUYV_ANY
                            else ": pv_hdr_views does not read YUV 4:2:2 / 4:4:4" if src_layout in _YUV4_ANY else ""))
    return code, tone


# --------------------------------------------------------------------------- fused device path
def _affine(mean, std, div255, channels, device):
    """(ch_scale, ch_shift) of Div255 + Normalize as fp32 device tensors, or (None, None)."""
    if mean is None and std is None and not div255:
        return None, None
    mean_t = torch.tensor(mean if mean is not None else [0.0] * channels, dtype=torch.float64)
    std_t = torch.tensor(std if std is not None else [1.0] * channels, dtype=torch.float64)
    if mean_t.numel() != channels or std_t.numel() != channels:
        raise ValueError("mean/std must have %d entries" % channels)
    k = 255.0 if div255 else 1.0
    return (1.0 / (k * std_t)).float().to(device), (-mean_t / std_t).float().to(device)


def _views(spatial_idx):
    views = (spatial_idx,) if isinstance(spatial_idx, int) else tuple(spatial_idx)
    if not 1 <= len(views) <= 3 or any(v not in (0, 1, 2) for v in views):
        raise ValueError("spatial_idx is 0, 1 or 2, or a tuple of up to three of them; got %r" % (spatial_idx,))
    return views


def _source_geometry(clip, src_layout):
    """(B, C, T, Hs, Ws) of a clip in either source layout."""
    if clip.dim() != 5:
        raise RuntimeError("expected a 5-d %s clip, got %s" % (src_layout, tuple(clip.shape),))
    if src_layout == "NCTHW":
        return tuple(clip.shape)
    b, t, h, w, c = clip.shape
    return b, c, t, h, w


def _view_geometry(hs, ws, short_side, crop, views, what=""):
    """(Hn, Wn, [(y_off, x_off) per view]) of the views of an Hs x Ws source: short_side_scale, then uniform_crop.  `crop` is
    the side of the square crop, or a pair (Ho, Wo): NO crop -- the window is the whole scaled frame, which must then be
    exactly Ho x Wo.  RuntimeError, its message behind `what`, if the window does not fit."""
    hn, wn = scaled_size(hs, ws, short_side)
    if isinstance(crop, (tuple, list)):
        if (hn, wn) != (int(crop[0]), int(crop[1])):
            raise RuntimeError("%sthe %d x %d frame scales to %d x %d, the deploy form takes %d x %d and nothing is cropped"
                               % (what, hs, ws, hn, wn, crop[0], crop[1]))
        return hn, wn, [(0, 0)] * len(views)
    if crop > hn or crop > wn:
        raise RuntimeError("%sa %d crop does not fit the %d x %d frame scaled to %d x %d" % (what, crop, hs, ws, hn, wn))
    return hn, wn, [crop_offsets(hn, wn, crop, v) for v in views]


def _set_views(d, hn, wn, offsets, crop_size=None):
    """The view fields of a descriptor, or (`crop_size` None) of a ViewSource record, whose window is its launch's."""
    d.Hn, d.Wn = hn, wn
    for i, (y, x) in enumerate(offsets):
        d.y_off[i], d.x_off[i] = y, x
    if crop_size is not None:
        d.Ho, d.Wo, d.n_views = crop_size, crop_size, len(offsets)


def _set_affine(d, scale, shift):
    """The affine pair of `_affine` into a descriptor; (None, None) leaves the null pointers: no map."""
    if scale is not None:
        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()


def _src_codes(src_layout, dtype):
    """(src_layout, src_dtype) as the descriptors code them; `dtype` is the tensors' and decides for RGB / planar sources."""
    from . import _lib as L
    if src_layout in _YUV_ANY:
        code = (L.SRC_YUV422 if src_layout in YUV422_LAYOUTS else L.SRC_YUV444 if src_layout in YUV444_LAYOUTS
                else L.SRC_YUYV422 if src_layout in _YUYV_ANY else L.SRC_YUV420)
        return code, L.PV_U16 if src_layout in _YUV_WIDE else L.PV_U8
    if src_layout in _PACKED_ANY:
        return getattr(L, "SRC_" + _packed_name(src_layout)), L.PV_U8
    return L.SRC_NCTHW if src_layout == "NCTHW" else L.SRC_NTHWC, L.PV_U8 if dtype == torch.uint8 else L.PV_F32


def _rgb_source(d, src, src_layout, c, hs, ws, geo, crop_size):
    """What a ResampleDesc and a VideoViewsDesc share: the RGB / planar source `src` of C x Hs x Ws frames and the views
    (`geo`: `_view_geometry`) of short_side_scale + uniform_crop.  Returns `d`."""
    d.src, d.C, d.Hs, d.Ws = src.data_ptr(), c, hs, ws
    d.src_layout, d.src_dtype = _src_codes(src_layout, src.dtype)
    _set_views(d, *geo, crop_size)
    return d


def _resample_desc(clip, src_layout, short_side, crop_size, views):
    """A ResampleDesc with the source and the geometry of short_side_scale + uniform_crop filled in (the destination, the
    frame selection and the affine map are the caller's).  `clip` is contiguous, uint8 or fp32, on the device."""
    from . import _lib as L
    b, c, t, hs, ws = _source_geometry(clip, src_layout)
    d = _rgb_source(L.ResampleDesc(), clip, src_layout, c, hs, ws, _view_geometry(hs, ws, short_side, crop_size, views), crop_size)
    d.B, d.T, d.src_T = b, t, t
    return d


def _device_source(clip, device):
    clip = clip.to(device, non_blocking=True)
    if clip.dtype not in (torch.uint8, torch.float32):
        clip = clip.float()
    return clip.contiguous()


def _video_geometry(video, src_layout):
    """(C, N, Hs, Ws) of ONE video: [C,N,H,W] ("NCTHW") or the decoder's [N,H,W,3] ("NTHWC")."""
    if video.dim() != 4:
        raise RuntimeError("expected one 4-d %s video, got %s" % (src_layout, tuple(video.shape),))
    if src_layout == "NCTHW":
        return tuple(video.shape)
    n, h, w, c = video.shape
    return c, n, h, w


def _on_device(video, device, what):
    if video.device.type != device.type or (device.index is not None and video.device.index != device.index):
        raise RuntimeError("%s is on %s, the deploy form on %s" % (what, video.device, device))


def _video_source(video, src_layout, device, coded_height=None, height=None, what="the video"):
    """What a legal video tensor is for `src_layout`, for `fill_video` and `video_batch` alike: on `device`, and either
    contiguous uint8 / fp32 [C,N,H,W], contiguous uint8 [N,H,W,3], YUV frames with the strides `yuv_geometry` accepts, or
    packed pixels [N,H,W,PB] with the strides `packed_geometry` accepts (a ValueError naming the stride otherwise).
    Returns (C, N, Hs, Ws, geom), `geom` being `yuv_geometry` / `packed_geometry` of the frames, or None.  RuntimeError, naming `what`, if not."""
    _on_device(video, device, what)
    if src_layout in _YUV_ANY:
        geom = yuv_geometry(video, src_layout, coded_height, height)
        return 3, geom["N"], geom["Hs"], geom["Ws"], geom
    if src_layout in _PACKED_ANY:                                # read where it lies: strides checked, never copied
        if video.dim() != 4:
            raise RuntimeError("expected one 4-d %s video, got %s" % (src_layout, tuple(video.shape),))
        geom = packed_geometry(video, src_layout)
        return 3, geom["N"], geom["Hs"], geom["Ws"], geom
    c, nf, hs, ws = _video_geometry(video, src_layout)
    if not video.is_contiguous() or video.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("%s is not a contiguous uint8 or fp32 tensor" % what)
    if src_layout == "NTHWC" and (c != 3 or video.dtype != torch.uint8):
        raise RuntimeError("a frame-interleaved video is uint8 [N,H,W,3], got %s %s" % (video.dtype, tuple(video.shape)))
    return c, nf, hs, ws, None


def pathway_tables(table, pathway_frames, num_frames):
    """The frame table of every input pathway from the table of the clip itself (`data.clip_frame_table`): pathway p holds
    the columns `temporal_indices(T, pathway_frames[p])` of the [n_clips, T] table -- uniform_temporal_subsample_repeated on
    frame numbers, so SlowFast's slow table is a column subset of the fast one.  Host int32 tensors; the check that every
    entry names a frame of the video is made HERE (the kernel only clamps), ValueError otherwise."""
    table = torch.as_tensor(table)
    if table.dim() != 2 or table.numel() == 0 or table.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16):
        raise ValueError("a frame table is a non-empty integer [n_clips, T] tensor, got %s %s" % (table.dtype, tuple(table.shape)))
    table = table.to("cpu", torch.int64)
    if int(table.min()) < 0 or int(table.max()) >= num_frames:
        raise ValueError("frame table entries %d..%d leave the video's frames [0, %d)"
                         % (int(table.min()), int(table.max()), num_frames))
    t = table.shape[1]
    return [table[:, temporal_indices(t, tp)].to(torch.int32).contiguous() for tp in pathway_frames]


def _yuv_desc(frames, geom, table, matrix, short_side, crop_size, views, geo=None):
    """A YuvViewsDesc with the source, the frame table, the conversion and the geometry of short_side_scale + uniform_crop
    filled in (destination, item range and affine map are the caller's).  `frames`, `table` (int32 [n_clips, T]) and
    `matrix` (fp32 [12]) are on the device and stay alive until the launch has run.  `geo`: the `_view_geometry` of the
    source, where the caller has it already."""
    from . import _lib as L
    d = L.YuvViewsDesc()
    _set_views(d, *(geo or _view_geometry(geom["Hs"], geom["Ws"], short_side, crop_size, views)), crop_size)
    d.src, d.t_index, d.yuv2rgb = frames.data_ptr(), table.data_ptr(), matrix.data_ptr()
    d.n_clips, d.T, d.N, d.t_stride = table.shape[0], table.shape[1], geom["N"], table.stride(0)
    for k in ("Hs", "Ws") + _YUV_PLANE_FIELDS + ("c_step",):
        setattr(d, k, geom[k])
    return d


def _clip_rows(n_clips, clip_frames, num_frames):
    """The frame table of B materialised clips of T' frames laid out as one sequence: row b = b * T' + the frames
    uniform_temporal_subsample picks (int32 [B, num_frames], host)."""
    idx = temporal_indices(clip_frames, num_frames)
    return (torch.arange(n_clips)[:, None] * clip_frames + idx[None, :]).to(torch.int32).contiguous()


def _scale_crop_launch(d, entry, what, b, c, affine, dtype, device, outer=None):
    """The tail of `device_scale_crop` for either kind of source: the planar [b * n_views, c, T, Ho, Wo] destination of
    `dtype`, the affine map (`affine`: mean, std, div255) and the launch of `entry` on `device`'s current stream (on `outer`,
    the descriptor that embeds `d`, when given)."""
    import ctypes as C
    from . import _lib as L
    scale, shift = _affine(*affine, c, device)
    _set_affine(d, scale, shift)
    out = torch.empty((b * d.n_views, c, d.T, d.Ho, d.Wo), dtype=dtype, device=device)
    d.dst, d.dst_layout = out.data_ptr(), L.DST_NCTHW
    d.dst_dtype = L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32
    with torch.cuda.device(device):
        L.check(getattr(L.lib(), entry)(C.byref(d if outer is None else outer),
                                        C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), what)
    return out


def _device_scale_crop_yuv(frames, short_side, crop_size, views, affine, num_frames, dtype, src_layout, yuv, coded_height, height,
                           hdr=None):
    device = frames.device if frames.is_cuda else torch.device("cuda", torch.cuda.current_device())
    frames = frames.to(device, non_blocking=True)
    geom = yuv_geometry(frames, src_layout, coded_height, height)
    b, t_src = (1, frames.shape[0]) if frames.dim() == 3 else tuple(frames.shape[:2])
    table = _clip_rows(b, t_src, num_frames if num_frames is not None else t_src).to(device)
    matrix = _yuv_matrix_of(yuv, src_layout).float().reshape(12).to(device)
    if hdr is not None:                                    # the clips as ONE source of pv_hdr_views, row b of the table per clip
        geo = _view_geometry(geom["Hs"], geom["Ws"], short_side, crop_size, views)
        src = HdrVideoSource(frames, geom, geo, b, len(views), device)
        h = src.desc(table, matrix, src_layout, (crop_size, crop_size), (hdr[0], hdr[1].to(device)), 0, b * len(views))
        return _scale_crop_launch(h.frames.batch, "pv_hdr_views", "hdr_views", b, 3, affine, dtype, device, outer=h)
    d = _yuv_desc(frames, geom, table, matrix, short_side, crop_size, views)
    entry = "pv_yuv16_views" if src_layout in YUV16_LAYOUTS else "pv_yuv_views"
    return _scale_crop_launch(d, entry, "yuv_views", b, 3, affine, dtype, device)


# --------------------------------------------------------------------------- frame-list sources (pv_frame_views)
class FrameList:
    """One video as a sequence of per-frame device tensors -- a decoder's surface pool, or the frames of a live stream --
    for `DevicePacker.video_batch` and the predictors of `inference`: the ingest reads every frame where it lies
    (`pv_frame_views`), nothing is stacked first.

    The frames share one device, dtype, shape and set of strides.  Per frame, by the packer's source layout: "NTHWC" a
    contiguous uint8 [H, W, 3]; "NCTHW" a contiguous uint8 or fp32 [C, H, W]; the YUV layouts a uint8 (`YUV16_LAYOUTS`:
    uint16 or int16) 2-d [Hc*3/2, W] with stride(1) == 1 and any row pitch P >= W (`yuv_geometry` of a one-frame view: the surface is the Hc*3/2 * P bytes from
    its first sample -- the half-pitch chroma rows of I420 / YV12 lie partly behind column W).  `src_layout`, when given,
    checks that form at construction; `video_batch` checks it in any case.  The packed layouts (`PACKED_LAYOUTS`): a uint8
    [H, W, PB] with stride(-1) == 1, stride(-2) == PB and any row stride >= W * PB (`packed_geometry`).  The packed 4:2:2 layouts
    (`YUYV_LAYOUTS`): a uint8 (Y21x: uint16 or int16) [H, W, 2] with stride(-1) == 1, stride(-2) == 2 and any row stride >= 2 * W
    (`yuyv_geometry`) -- what `cv2.VideoCapture.read()` returns with CAP_PROP_CONVERT_RGB = 0.  A frame may be a view at any offset inside a
    larger buffer and appear more than once, and the frames may have been allocated in any order.  The list keeps its
    tensors alive; `len()` is the frame count; `stack(src_layout)` is the contiguous video the frames make up."""

    def __init__(self, frames, src_layout=None):
        frames = list(frames)
        if not frames:
            raise ValueError("a FrameList holds at least one frame")
        f0 = frames[0]
        for i, f in enumerate(frames):
            if not isinstance(f, torch.Tensor):
                raise TypeError("frame %d is a %s, not a tensor" % (i, type(f).__name__))
            for what, a, b in (("device", f.device, f0.device), ("dtype", f.dtype, f0.dtype),
                               ("shape", tuple(f.shape), tuple(f0.shape)), ("strides", f.stride(), f0.stride())):
                if a != b:
                    raise RuntimeError("the frames of a FrameList share one device, dtype, shape and set of strides: "
                                       "frame %d has %s %s, frame 0 %s" % (i, what, a, b))
        self.frames = frames
        self.device, self.dtype, self.shape = f0.device, f0.dtype, tuple(f0.shape)
        if src_layout is not None:
            self.geometry(src_layout)

    def __len__(self):
        return len(self.frames)

    def geometry(self, src_layout, coded_height=None, height=None):
        """(C, Hs, Ws, geom) of one frame in `src_layout`, `geom` being `yuv_geometry` of a one-frame view for the YUV
        layouts (frame_stride: the extent of one frame) and None otherwise.  RuntimeError for a frame of another form."""
        f = self.frames[0]
        if src_layout in _YUV_ANY:
            if src_layout in _YUYV_ANY:
                if f.dim() != 3:
                    raise RuntimeError("a %s frame is [H, W, 2] (uint8; Y210 / Y212 / Y216: uint16 or int16), got %s %s"
                                       % (src_layout, f.dtype, tuple(f.shape)))
                geom = yuyv_geometry(f, src_layout)
                return 3, geom["Hs"], geom["Ws"], geom
            if f.dim() != 2:
                raise RuntimeError("a %s frame is 2-d: uint8 [Hc*3/2, W] (4:2:2: [Hc*2, W], 4:4:4: [Hc*3, W]; 16-bit layouts: uint16 "
                                   "or int16), got %s %s" % (src_layout, f.dtype, tuple(f.shape)))
            geom = yuv_geometry(f[None], src_layout, coded_height, height)
            return 3, geom["Hs"], geom["Ws"], geom
        if src_layout in _PACKED_ANY:
            if f.dim() != 3:
                raise RuntimeError("a %s frame is uint8 [H, W, %d], got %s %s" % (src_layout, _packed_bytes(src_layout), f.dtype, tuple(f.shape)))
            geom = packed_geometry(f, src_layout)
            return 3, geom["Hs"], geom["Ws"], geom
        if src_layout not in ("NCTHW", "NTHWC"):
            raise ValueError(_LAYOUT_ERROR)
        if f.dim() != 3 or not f.is_contiguous() or f.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError("a frame of a FrameList is a contiguous uint8 or fp32 [H,W,3] / [C,H,W] tensor, got %s %s with "
                               "strides %s" % (f.dtype, tuple(f.shape), f.stride()))
        if src_layout == "NCTHW":
            return f.shape[0], f.shape[1], f.shape[2], None
        if f.shape[2] != 3 or f.dtype != torch.uint8:
            raise RuntimeError("a frame-interleaved frame is uint8 [H,W,3], got %s %s" % (f.dtype, tuple(f.shape)))
        return 3, f.shape[0], f.shape[1], None

    def stack(self, src_layout="NTHWC"):
        """The contiguous video: [N,H,W,3], [C,N,H,W] ("NCTHW") or [N, Hc*3/2, W] (a YUV layout, pitch W)."""
        return torch.stack(self.frames, dim=1 if src_layout == "NCTHW" else 0)


def _refuse_orientation(orientation, what):
    if _orient(0 if orientation is None else orientation):
        raise RuntimeError("%s reads materialised clips through the one-source entry points, which have no orientation; a "
                           "turned or mirrored video is read in place by DevicePacker.video_batch(..., orientation=) / "
                           "fill_batch (inference.VideoPredictor and its kin take orientation= too)" % what)


INTERPOLATIONS = ("bilinear", "area")


def _interpolation(interpolation, orientation=None, hdr=None, what="the device ingest"):
    """`interpolation` as every device entry point takes it: "bilinear" (the four-tap blend of `pv_resample_crop`) or "area"
    (the box filter of `pv_area_views`: F.interpolate(mode="area"), the downscale mode for 720p and larger sources).  Returns
    whether it is "area"; ValueError for any other string, and for "area" together with what `pv_area_views` does not carry:
    a non-zero `orientation` (one code or one per video) and `hdr`."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError("%s: interpolation is 'bilinear' or 'area', got %r" % (what, interpolation))
    if interpolation != "area":
        return False
    codes = orientation if isinstance(orientation, (list, tuple)) else [orientation]
    if any(_orient(0 if o is None else o) for o in codes):
        raise ValueError("%s: interpolation='area' reads upright records only (pv_area_views): orientation is not supported "
                         "together with it" % what)
    if hdr is not None:
        raise ValueError("%s: interpolation='area' has no PQ / HLG tap map (pv_area_views): hdr is not supported together "
                         "with it" % what)
    return True


def _refuse_frames(video, what):
    if isinstance(video, FrameList):
        raise RuntimeError("%s takes one tensor; a FrameList goes through video_batch / fill_batch" % what)


# --------------------------------------------------------------------------- many videos per forward (pv_batch_views)
def batch_items(clips_per_video, n_views):
    """The video-major item sequence of a batch of videos: video j, then `clip * n_views + v`.  Returns (items, video_of,
    clip_of, row0): `items` int32 [total, 4] = (source, row, view, 0) as `pv_view_item` holds them, `row` counting the rows
    of the CONCATENATED frame table; `video_of` / `clip_of` int32 [total] = the video and the concatenated-table row of
    every item; `row0[j]` = the first row of video j."""
    counts = [int(c) for c in clips_per_video]
    if not counts or any(c <= 0 for c in counts) or n_views < 1:
        raise ValueError("a batch holds at least one video, and every video at least one clip; got %s clips x %d views" % (counts, n_views))
    row0 = [0]
    for c in counts[:-1]:
        row0.append(row0[-1] + c)
    video_of = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts) * n_views)
    clip_of = torch.arange(sum(counts), dtype=torch.int32).repeat_interleave(n_views)
    view = torch.arange(n_views, dtype=torch.int32).repeat(sum(counts))
    items = torch.stack([video_of, clip_of, view, torch.zeros_like(view)], dim=1).contiguous()
    return items, video_of, clip_of, row0


def batch_chunks(total, batch):
    """[(i0, n)] of the forwards that walk `total` items in chunks of the deploy batch; only the last one may be short."""
    return [(i0, min(batch, total - i0)) for i0 in range(0, total, batch)]


def batch_tables(tables, pathway_frames, nums_frames):
    """The per-pathway frame tables of a batch of videos, the videos' rows one after another: `pathway_tables` of every
    video's [n_clips_j, T] table -- checked against THAT video's frame count -- concatenated per pathway (host int32)."""
    if len(tables) != len(nums_frames) or not tables:
        raise ValueError("%d frame tables for %d videos" % (len(tables), len(nums_frames)))
    per_video = [pathway_tables(t, pathway_frames, n) for t, n in zip(tables, nums_frames)]
    return [torch.cat([pv[p] for pv in per_video]).contiguous() for p in range(len(pathway_frames))]


class VideoBatch:
    """What `DevicePacker.video_batch` uploaded for a list of videos: the `pv_view_source` records and the `pv_view_item`
    sequence (host copies and the device copies of the same bytes), the concatenated per-pathway frame tables, and the
    videos themselves, kept alive.  `total` items; `video_of` / `clip_of` (int32, device) = the video and the row of the
    concatenated table behind every item; `clips[j]` / `row0[j]` = the clips of video j and its first row.  For videos
    given as `FrameList`s `frame_ptrs` (host int64, video-major: the frame addresses of video j from `frame_first[j]` on)
    and `frame_ptrs_dev`, the same bytes on the device, are the pointer table of `pv_frame_views`, and the `src` of record j
    is the device address of its slice; for tensors they are None.  `regions` / `regions_dev`: the per-pathway rectangle
    tables of `pv_region_views` for a batch built with `regions=`, else None."""

    def __init__(self, videos, sources, items, items_t, tables, video_of, clip_of, clips, row0, n_views, src_dtype, upload,
                 frame_ptrs=None, frame_ptrs_dev=None, frame_first=None, regions=None):
        self.frame_ptrs, self.frame_ptrs_dev, self.frame_first = frame_ptrs, frame_ptrs_dev, frame_first
        # per pathway the `pv_view_region` records of every (table row, destination frame) -- host int32 [n_rows, T_p, 8] and the
        # same bytes on the device --, or None: the views are the records' own
        self.regions = regions
        self.regions_dev = None if regions is None else [upload(r) for r in regions]
        self.videos, self.sources, self.items = list(videos), sources, items
        self.n_views, self.src_dtype, self.clips, self.row0 = n_views, src_dtype, list(clips), list(row0)
        self.total, self.n_rows = len(items), sum(clips)
        # the very buffers the descriptors point at are the ones uploaded
        self.sources_dev = upload(torch.frombuffer(sources, dtype=torch.uint8))
        self.items_dev = upload(torch.frombuffer(items, dtype=torch.uint8))
        self.tables = [upload(t) for t in tables]
        self.video_of, self.clip_of = upload(video_of), upload(clip_of)
        self.item_rows = items_t                   # host int32 [total, 4]: (source, row, view, 0)


def region_records(regions, window):
    """The `pv_view_region` records of validated rectangles [..., 4] (`_check_regions`) for a launch whose window is
    `window` = (Ho, Wo): a contiguous host int32 tensor [..., 8] holding, per rectangle, top, left, h, w, the BITS of
    sy = (float)h / (float)Ho and sx = (float)w / (float)Wo -- divided in fp32, as the library divides -- and two zeros."""
    ho, wo = window
    rec = torch.zeros(tuple(regions.shape[:-1]) + (8,), dtype=torch.int32)
    rec[..., :4] = regions.to(torch.int32)
    rec[..., 4] = (regions[..., 2].to(torch.float32) / torch.tensor(float(ho), dtype=torch.float32)).view(torch.int32)
    rec[..., 5] = (regions[..., 3].to(torch.float32) / torch.tensor(float(wo), dtype=torch.float32)).view(torch.int32)
    return rec.contiguous()


def build_video_batch(videos, tables, src_layout, short_side, crop_size, views, pathway_frames, channels, device, upload,
                      height=None, coded_height=None, orientation=None, regions=None):
    """The host half of `DevicePacker.video_batch` (see there): validate every video, build the records, the item sequence
    and the concatenated tables, and hand them to `upload` (host tensor -> device tensor) once.  `crop_size` is the side of
    the square crop, or a pair (Ho, Wo): NO crop -- the window is the whole scaled frame, and every video must scale to
    exactly Ho x Wo.  The videos are all tensors or all `FrameList`s; for `FrameList`s ONE int64 table of frame addresses,
    video-major, is uploaded in front of the records, and record j points at its slice of the device copy.
    `orientation`: one code (`orientation_code`) or one per video, None = 0 -- the videos are the STORED frames, as a decoder
    hands them out; the record keeps the stored sizes and carries the code, and the views are cut from the displayed frame.
    `regions`: one integer tensor [n_clips_j, clip_frames, 4] of (top, left, h, w) per video, aligned with `tables[j]` -- every
    destination frame is the resize of ITS rectangle of ITS source frame to `crop_size` = (Ho, Wo) (`pv_region_views`); there
    is then no short-side scale (`short_side` is not read), one view, and no orientation.  Pathway p gets the columns of the
    rectangle table that `pathway_tables` gives it of the frame table."""
    from . import _lib as L
    videos = list(videos)
    if regions is not None:
        regions = list(regions)
        if len(regions) != len(videos):
            raise ValueError("%d region tables for %d videos" % (len(regions), len(videos)))
        if len(views) != 1:
            raise ValueError("regions are resized whole: one view, not %d" % len(views))
        window = _size_pair(crop_size, "crop_size")
    if not videos or len(tables) != len(videos):
        raise ValueError("%d frame tables for %d videos" % (len(tables), len(videos)))
    as_frames = isinstance(videos[0], FrameList)
    if any(isinstance(v, FrameList) != as_frames for v in videos):
        raise ValueError("the videos of one call are all tensors or all FrameLists, not a mix of tensors and FrameLists "
                         "(wrap a tensor: FrameList(video.unbind(0)))")
    is_yuv = src_layout in _YUV_ANY

    def per_video(x, what):
        if x is None or not isinstance(x, (list, tuple)):
            return [None if x is None else int(x)] * len(videos)         # any integer type: int, numpy, a 0-d tensor
        x = list(x)
        if len(x) != len(videos):
            raise ValueError("%s is one number or one per video: %d for %d videos" % (what, len(x), len(videos)))
        return x

    heights, coded = per_video(height, "height"), per_video(coded_height, "coded_height")
    orients = [_orient(0 if o is None else o) for o in per_video(orientation, "orientation")]
    if regions is not None and any(orients):
        raise ValueError("regions are rectangles of the STORED frame and pv_region_views reads upright records only: "
                         "orientation is not supported together with regions")
    sources = (L.ViewSource * len(videos))()
    nums_frames, dtype = [], videos[0].dtype
    for j, video in enumerate(videos):
        what, rec = "video %d" % j, sources[j]
        if as_frames:
            _on_device(video, device, what)
            (c, hs, ws, geom), nf = video.geometry(src_layout, coded[j], heights[j]), len(video)
        else:
            if is_yuv and video.dim() != 1 + _yuv_dims(src_layout):
                raise RuntimeError("video %d: expected one %d-d %s video, got %s" % (j, 1 + _yuv_dims(src_layout), src_layout, tuple(video.shape)))
            c, nf, hs, ws, geom = _video_source(video, src_layout, device, coded[j], heights[j], what)
        if (as_frames or not is_yuv) and video.dtype != dtype:
            raise RuntimeError("the videos of one batch have one dtype: video %d is %s, video 0 %s" % (j, video.dtype, dtype))
        if c != channels:
            raise RuntimeError("video %d has %d channels, the deploy form takes %d" % (j, c, channels))
        for k in _YUV_PLANE_FIELDS if geom is not None else ():   # YUV planes; packed pixels: the row pitch and the frame stride
            setattr(rec, k, geom[k])
        hd, wd = displayed_size(hs, ws, orients[j])               # the views are cut from the displayed frame
        if regions is not None:                                   # the geometry is per frame; the record's own is not read
            hn, wn, offsets = window[0], window[1], [(0, 0)]
            regions[j] = _check_regions(regions[j], hs, ws, region_evenness(src_layout), what + ": regions")
        else:
            hn, wn, offsets = _view_geometry(hd, wd, short_side, crop_size, views, what + ": ")
        _set_views(rec, hn, wn, offsets)
        rec.src, rec.N, rec.Hs, rec.Ws = (None if as_frames else video.data_ptr()), nf, hs, ws
        if orients[j]:                                            # default records keep the zero they were built with
            rec.orient = orients[j]
        # (float)Hd / (float)Hn: sizes are exact in fp32, and a double quotient rounded once more to fp32 IS the fp32 quotient
        rec.sy, rec.sx = hd / hn, wd / wn
        nums_frames.append(nf)
    clip_frames = None
    for j, t in enumerate(tables):
        t = torch.as_tensor(t)
        if t.dim() == 2 and clip_frames is None:
            clip_frames = t.shape[1]
        if t.dim() != 2 or t.shape[1] != clip_frames:
            raise ValueError("video %d: a frame table is [n_clips, %s], got %s" % (j, clip_frames, tuple(t.shape)))
    cat = batch_tables(tables, pathway_frames, nums_frames)       # range-checks every table against ITS video
    clips = [int(torch.as_tensor(t).shape[0]) for t in tables]
    region_tables = None
    if regions is not None:
        for j, r in enumerate(regions):
            if tuple(r.shape) != (clips[j], clip_frames, 4):
                raise ValueError("video %d: a region table is [n_clips, clip_frames, 4] = [%d, %d, 4] like its frame table, got %s"
                                 % (j, clips[j], clip_frames, tuple(r.shape)))
        whole = torch.cat(regions)                                # [n_rows, clip_frames, 4]: the rows of all videos
        region_tables = [region_records(whole[:, temporal_indices(clip_frames, tp)], window) for tp in pathway_frames]
    items_t, video_of, clip_of, row0 = batch_items(clips, len(views))
    items = (L.ViewItem * items_t.shape[0]).from_buffer_copy(items_t.numpy().tobytes())
    src_dtype = _src_codes(src_layout, dtype)[1]
    if not as_frames:
        return VideoBatch(videos, sources, items, items_t, cat, video_of, clip_of, clips, row0, len(views), src_dtype, upload,
                          regions=region_tables)
    # the pointer table of the call: the frame addresses of video j from first[j] on; the records point into the DEVICE copy
    ptrs = torch.tensor([f.data_ptr() for video in videos for f in video.frames], dtype=torch.int64)
    first = [0]
    for n in nums_frames[:-1]:
        first.append(first[-1] + n)
    ptrs_dev = upload(ptrs)
    for rec, k in zip(sources, first):
        rec.src = ptrs_dev.data_ptr() + 8 * k
    return VideoBatch(videos, sources, items, items_t, cat, video_of, clip_of, clips, row0, len(views), src_dtype, upload,
                      ptrs, ptrs_dev, first, regions=region_tables)


class HdrVideoSource:
    """ONE upright video (or the frame sequence of B materialised clips) as the single record of `pv_hdr_views` launches: the
    `pv_view_source` record and the video-major item sequence of its `n_clips` x `n_views` views, on the host and -- the very
    same bytes -- on the device, built and uploaded once; `desc` is the descriptor of a window of that sequence.  The paths
    that launch the one-source `pv_yuv16_views` for `hdr=None` run through this: that entry point has no tap map."""

    def __init__(self, frames, geom, geo, n_clips, n_views, device):
        from . import _lib as L
        hn, wn, offsets = geo
        self.frames, self.n_clips, self.n_views = frames, n_clips, n_views
        self.sources = (L.ViewSource * 1)()
        rec = self.sources[0]
        for k in _YUV_PLANE_FIELDS:
            setattr(rec, k, geom[k])
        _set_views(rec, hn, wn, offsets)
        rec.src, rec.N, rec.Hs, rec.Ws = frames.data_ptr(), geom["N"], geom["Hs"], geom["Ws"]
        rec.sy, rec.sx = geom["Hs"] / hn, geom["Ws"] / wn          # as build_video_batch divides
        items_t = batch_items([n_clips], n_views)[0]
        self.items = (L.ViewItem * items_t.shape[0]).from_buffer_copy(items_t.numpy().tobytes())
        self.sources_dev = torch.frombuffer(self.sources, dtype=torch.uint8).to(device)
        self.items_dev = torch.frombuffer(self.items, dtype=torch.uint8).to(device)
        self.key = self.key_of(frames, geom, geo, n_clips, n_views)

    @staticmethod
    def key_of(frames, geom, geo, n_clips, n_views):
        """What the record and the item sequence depend on: two videos with one key share them."""
        return (frames.data_ptr(), tuple(sorted(geom.items())), geo[0], geo[1], tuple(geo[2]), n_clips, n_views)

    def desc(self, table, matrix, src_layout, window, hdr, item0, n_items):
        """The HdrViewsDesc of items [item0, item0 + n_items) (destination and affine map are the caller's); `table` int32
        [n_clips, T], `matrix` fp32 [12] and the tone table `hdr[1]` are on the device and stay alive until the launch has
        run (the descriptor's `keep` holds them)."""
        import ctypes as C
        from . import _lib as L
        h = L.HdrViewsDesc()
        d = h.frames.batch
        d.sources, d.sources_dev = C.addressof(self.sources), self.sources_dev.data_ptr()
        first = min(item0, len(self.items) - 1) * C.sizeof(L.ViewItem)      # n_items == 0: any valid address, never read
        d.items, d.items_dev = C.addressof(self.items) + first, self.items_dev.data_ptr() + first
        d.t_index, d.n_rows, d.t_stride = table.data_ptr(), table.shape[0], table.stride(0)
        d.n_sources, d.n_items, d.C, d.T = 1, n_items, 3, table.shape[1]
        d.src_layout, d.src_dtype = _src_codes(src_layout, None)
        d.c_step, d.yuv2rgb = _yuv_c_step(src_layout), matrix.data_ptr()
        d.Ho, d.Wo, d.n_views = window[0], window[1], self.n_views
        h.transfer, h.tone = hdr[0], hdr[1].data_ptr()
        h.keep = (self, table, matrix, hdr[1])
        return h


def _batch_launch_fields(d, batch, table, item0, n_items, channels, src_layout, matrix, window):
    """The fields of a BatchViewsDesc that say WHAT a launch over items [item0, item0 + n_items) of `batch` (a `VideoBatch`)
    reads and how large it writes: records, item window, the device frame table `table` [n_rows, T], the source form and the
    window (Ho, Wo).  Destination and affine map are the caller's."""
    import ctypes as C
    from . import _lib as L
    d.sources, d.sources_dev = C.addressof(batch.sources), batch.sources_dev.data_ptr()
    first = min(item0, batch.total - 1) * C.sizeof(L.ViewItem)      # n_items == 0: any valid address, never read
    d.items, d.items_dev = C.addressof(batch.items) + first, batch.items_dev.data_ptr() + first
    d.t_index, d.n_rows, d.t_stride = table.data_ptr(), table.shape[0], table.stride(0)
    d.n_sources, d.n_items, d.C, d.T = len(batch.sources), n_items, channels, table.shape[1]
    d.src_layout, d.src_dtype = _src_codes(src_layout, None)[0], batch.src_dtype
    if src_layout in _YUV_ANY:
        d.c_step, d.yuv2rgb = _yuv_c_step(src_layout), matrix.data_ptr()
    d.Ho, d.Wo, d.n_views = window[0], window[1], batch.n_views


@torch.no_grad()
def device_resized_crop(clip, regions, size, mean=None, std=None, div255=False, dtype=torch.bfloat16, src_layout="NCTHW",
                        yuv=("bt709", False), coded_height=None, height=None):
    """Normalize(Div255(resized_crop(clip[b], regions[b], size))) for every clip b in ONE launch of `pv_region_views`: a planar
    [B, C, T, Ho, Wo] tensor of `dtype` (bf16 or fp32) on the GPU.  `clip` is [B,C,T,H,W] ("NCTHW"; uint8 or float), the
    decoder's [B,T,H,W,3] uint8 ("NTHWC"), or -- the YUV 4:2:0 layouts of `device_scale_crop`, 8- and 16-bit -- [B, T, Hc*3/2, W]
    (or [T, Hc*3/2, W]: one clip) with the strides it has, converted tap by tap (`yuv`, `coded_height`, `height` as there).
    `regions` is an integer [B, T, 4] tensor of (top, left, h, w): a rectangle per frame (`box_regions`; even members for
    YUV); `size` an int or (Ho, Wo).  The clips are read where they lie: no crop, no RGB copy and no resized intermediate is
    made.  The transform alone, as `device_scale_crop` is; `resized_crop` is the host mirror."""
    from . import _lib as L
    if src_layout not in _SRC_LAYOUTS:
        raise ValueError(_LAYOUT_ERROR)
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("dtype is torch.bfloat16 or torch.float32")
    window = _size_pair(size)
    is_yuv = src_layout in _YUV_ANY
    if is_yuv and clip.dim() == 1 + _yuv_dims(src_layout):
        clip, regions = clip.unsqueeze(0), torch.as_tensor(regions).unsqueeze(0)
    if clip.dim() != (2 + _yuv_dims(src_layout) if is_yuv else 5):
        raise RuntimeError("expected %s clips [B, ...], got %s" % (src_layout, tuple(clip.shape),))
    if src_layout in _PACKED_ANY:                                # the stride rules, before any device is touched
        packed_geometry(clip[0], src_layout)
    if src_layout in _YUYV_ANY:
        yuyv_geometry(clip[0], src_layout)
    device = clip.device if clip.is_cuda else torch.device("cuda", torch.cuda.current_device())
    in_place = is_yuv or src_layout in _PACKED_ANY               # read with the strides they have: never copied
    clip = clip.to(device, non_blocking=True) if in_place else _device_source(clip, device)
    b, t = clip.shape[0], clip.shape[2] if src_layout == "NCTHW" else clip.shape[1]
    regions = torch.as_tensor(regions)
    if regions.dim() != 3 or tuple(regions.shape) != (b, t, 4):
        raise ValueError("regions are [B, T, 4] = [%d, %d, 4], a rectangle per frame of every clip; got %s" % (b, t, tuple(regions.shape)))
    channels = 3 if in_place else clip.shape[1 if src_layout == "NCTHW" else 4]
    frames = torch.arange(t, dtype=torch.int32)[None]
    # every clip a source of its own, its T frames one table row: the item-sourced launch of DevicePacker.fill_batch
    batch = build_video_batch(list(clip.unbind(0)), [frames] * b, src_layout, None, window, (1,), [t], channels, device,
                              lambda x: x.to(device), height, coded_height, None, [regions[j:j + 1] for j in range(b)])
    g = L.RegionViewsDesc()
    matrix = _yuv_matrix_of(yuv, src_layout).float().reshape(12).to(device) if is_yuv else None
    _batch_launch_fields(g.frames.batch, batch, batch.tables[0], 0, b, channels, src_layout, matrix, window)
    g.regions, g.regions_dev = batch.regions[0].data_ptr(), batch.regions_dev[0].data_ptr()
    return _scale_crop_launch(g.frames.batch, "pv_region_views", "region_views", b, channels, (mean, std, div255), dtype, device,
                              outer=g)


@torch.no_grad()
def device_scale_crop(clip, short_side, crop_size, spatial_idx=1, mean=None, std=None, div255=False, num_frames=None,
                      dtype=torch.bfloat16, src_layout="NCTHW", yuv=("bt709", False), coded_height=None, height=None,
                      orientation=0, hdr=None, interpolation="bilinear"):
    """uniform_crop(short_side_scale(Normalize(Div255(uniform_temporal_subsample(clip, num_frames))))) for every view of
    `spatial_idx` in one launch of `pv_resample_crop`: a planar [B * n_views, C, T, crop, crop] tensor of `dtype` (bf16 or
    fp32) on the GPU, item b * n_views + v being view v of clip b.  `clip` is [B,C,T,H,W] ("NCTHW"; uint8 or float) or the
    decoder's [B,T,H,W,3] uint8 ("NTHWC").

    With `src_layout` "NV12", "NV21", "I420" or "YV12" the clip is decoder-native YUV 4:2:0, uint8 [B, T, Hc*3/2, W] (or
    [T, Hc*3/2, W]: one clip) with the strides it has (`yuv_geometry`: `coded_height`, `height`), converted tap by tap inside
    the same launch (`pv_yuv_views`) by `yuv`: (standard, full_range) for `yuv_matrix`, or a 3 x 4 matrix.  With a layout of
    `YUV16_LAYOUTS` ("P010", "I010", ...) the clip is uint16 or int16 and read by `pv_yuv16_views`; a (standard, full_range)
    pair is composed with the layout's depth and bit alignment: `src_layout="P010", yuv=("bt2020", False)`.  `hdr` -- "pq",
    "hlg" or (transfer, `tone_params(...)`), for such a layout only -- maps every tap from BT.2020 PQ / HLG to BT.709 SDR
    before the blend, in the same launch (`pv_hdr_views`; `hdr_to_sdr` of `yuv420_to_rgb` is the host mirror).

    Materialised clips go through the one-source entry points, whose descriptors have no orientation: a non-zero
    `orientation` is refused; `DevicePacker.video_batch` reads turned and mirrored videos in place.

    With a layout of `PACKED_LAYOUTS` ("BGR", "RGBA", "BGRA", "ARGB", "ABGR"; "RGBX" and kin are aliases) the clip is uint8
    [B, T, H, W, PB] packed pixels with the strides it has (`packed_geometry`: a pitched surface is read in place, a
    ValueError names a stride that is not legal, nothing is ever made contiguous); every clip is a source of its own in one
    launch of `pv_batch_views`, and the result is bit for bit that of "NTHWC" on `packed_to_rgb(clip, layout).contiguous()`.

    With a layout of `YUV422_LAYOUTS` ("I422", "NV16", "I210", ...) or `YUV444_LAYOUTS` ("I444", "I410", ...) the clip is YUV
    4:2:2 [B, T, Hc*2, W] or 4:4:4 [B, T, Hc*3, W], uint8 or -- the 10- to 16-bit layouts -- uint16 / int16, with the strides it
    has (`yuv_geometry`); every clip is a source of its own in one launch of `pv_batch_views` (the one-source entry points read
    4:2:0 only), chroma is replicated over the pixels it covers and `yuv_to_rgb` is the host mirror.  `hdr` is a ValueError.

    With a layout of `YUYV_LAYOUTS` ("YUY2" -- alias "YUYV" --, "YVYU", "UYVY", "Y210" / "Y212" / "Y216") the clip is packed YUV
    4:2:2 [B, T, H, W, 2] (or [T, H, W, 2]: one clip), uint8 or -- Y21x -- uint16 / int16, with the strides it has (`yuyv_geometry`:
    a pitched surface or a column slice from an even column is read in place, a ValueError names a stride that is not legal);
    every clip is a source of its own in one launch of `pv_batch_views`, and the result is bit for bit that of "I422" / "I216"
    on `yuyv_to_planar(clip, layout)` with the same matrix.  `hdr` is a ValueError.

    `interpolation="area"` scales with the box filter of `short_side_scale(x, size, "area")` instead of four taps -- what a
    720p or larger source needs: every clip is a source of its own in ONE launch of `pv_area_views`, any source layout, up to
    three views; a ValueError together with a non-zero `orientation` or `hdr`, and for any other string."""
    area = _interpolation(interpolation, orientation, hdr, "device_scale_crop")
    _refuse_orientation(orientation, "device_scale_crop")
    if src_layout not in _SRC_LAYOUTS:
        raise ValueError(_LAYOUT_ERROR)
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("dtype is torch.bfloat16 or torch.float32")
    views = _views(spatial_idx)
    hdr = _hdr_of(hdr, src_layout)                             # ValueError for an 8-bit or RGB source
    # item-sourced launches: pv_area_views, or pv_batch_views for packed pixels and YUV 4:2:2 / 4:4:4
    if area or src_layout in _PACKED_ANY or src_layout in _YUV4_ANY:
        return _device_scale_crop_items(clip, short_side, crop_size, views, (mean, std, div255), num_frames, dtype, src_layout,
                                        yuv, coded_height, height, area)
    if src_layout in _YUV_ANY:
        return _device_scale_crop_yuv(clip, short_side, crop_size, views, (mean, std, div255), num_frames, dtype, src_layout,
                                      yuv, coded_height, height, hdr)
    _source_geometry(clip, src_layout)
    device = clip.device if clip.is_cuda else torch.device("cuda", torch.cuda.current_device())
    clip = _device_source(clip, device)
    d = _resample_desc(clip, src_layout, short_side, crop_size, views)
    if num_frames is not None and num_frames != d.src_T:
        index = temporal_indices(d.src_T, num_frames).to(torch.int32).to(device)
        d.T, d.t_index = num_frames, index.data_ptr()
    return _scale_crop_launch(d, "pv_resample_crop", "resample_crop", d.B, d.C, (mean, std, div255), dtype, device)


def _device_scale_crop_items(clip, short_side, crop_size, views, affine, num_frames, dtype, src_layout, yuv, coded_height, height,
                             area):
    """`device_scale_crop(interpolation="area")`, and `device_scale_crop` of packed pixels: every clip a source of its own, its
    frames one table row -- the item-sourced launch of `DevicePacker.fill_batch`, as `device_resized_crop` builds it -- and one
    launch of `pv_area_views` (`area`) or `pv_batch_views` (the one-source entry points do not read packed pixels)."""
    from . import _lib as L
    is_yuv = src_layout in _YUV_ANY
    in_place = is_yuv or src_layout in _PACKED_ANY               # read with the strides they have: never copied
    if is_yuv and clip.dim() == 1 + _yuv_dims(src_layout):
        clip = clip.unsqueeze(0)
    if clip.dim() != (2 + _yuv_dims(src_layout) if is_yuv else 5):
        raise RuntimeError("expected %s clips [B, ...], got %s" % (src_layout, tuple(clip.shape),))
    if src_layout in _PACKED_ANY:                                # the stride rules, before any device is touched
        packed_geometry(clip[0], src_layout)
    if src_layout in _YUYV_ANY:
        yuyv_geometry(clip[0], src_layout)
    device = clip.device if clip.is_cuda else torch.device("cuda", torch.cuda.current_device())
    clip = clip.to(device, non_blocking=True) if in_place else _device_source(clip, device)
    b, t_src = clip.shape[0], clip.shape[2] if src_layout == "NCTHW" else clip.shape[1]
    channels = 3 if in_place else clip.shape[1 if src_layout == "NCTHW" else 4]
    t = t_src if num_frames is None else num_frames
    frames = temporal_indices(t_src, t).to(torch.int32)[None]
    batch = build_video_batch(list(clip.unbind(0)), [frames] * b, src_layout, short_side, crop_size, views, [t], channels, device,
                              lambda x: x.to(device), height, coded_height)
    matrix = _yuv_matrix_of(yuv, src_layout).float().reshape(12).to(device) if is_yuv else None
    if not area:
        d = L.BatchViewsDesc()
        _batch_launch_fields(d, batch, batch.tables[0], 0, batch.total, channels, src_layout, matrix, (crop_size, crop_size))
        return _scale_crop_launch(d, "pv_batch_views", "batch_views", b, channels, affine, dtype, device)
    a = L.AreaViewsDesc()
    a.filter = L.PV_FILTER_AREA
    _batch_launch_fields(a.frames.batch, batch, batch.tables[0], 0, batch.total, channels, src_layout, matrix, (crop_size, crop_size))
    return _scale_crop_launch(a.frames.batch, "pv_area_views", "area_views", b, channels, affine, dtype, device, outer=a)


class DevicePacker:
    """`DevicePacker(deployed, mean, std, div255=True, frame_ratios=(4, 1))(clip)` = the deploy form
    applied to `[Normalize(Div255(subsample_r(clip))) for r in frame_ratios]`, with everything before
    the first convolution done by the ingest kernel.

    `deployed` is what `convert_to_deployable_form` returned for a whole model (one graph replay per
    forward); `frame_ratios` must be given for multi-pathway models in the order of the model's
    input list (SlowFast: slow = T/4 frames, fast = T frames), and left None for single-input models.
    A deployed detection model (DetectionBBoxNetwork) is called as `packer(clip, bboxes)`.

    With `short_side` and `crop_size` the packer also does `uniform_crop(short_side_scale(., short_side), crop_size, v)`
    for every v of `spatial_idx` (an int, or a tuple of up to three: the three-crop protocol) in the same pass
    (`pv_resample_crop`, one launch per pathway): `clip` may have any frame size and be [B,C,T,H,W] (`src_layout="NCTHW"`)
    or the decoder's uint8 [B,T,H,W,3] ("NTHWC"); the deploy form's batch is B * n_views, item b * n_views + v being view v
    of clip b (`VideoEnsembler`'s video_index for it is `repeat_interleave(n_views)`), and `crop_size` is the model's
    H == W.  The boxes of a detection model are given in the pixels of the SOURCE frame and follow the clip through
    `short_side_scale_with_boxes` and `uniform_crop_with_boxes` on the host (one view only).

    `src_layout` "NV12" / "NV21" / "I420" / "YV12": the clip is decoder-native YUV 4:2:0, uint8 [B, T, Hc*3/2, W] with the
    strides it has (`yuv_geometry`; `coded_height`, `height`), or one video [N, Hc*3/2, W] for `fill_video`; `yuv` is
    (standard, full_range) for `yuv_matrix` or a 3 x 4 matrix.  The ingest converts every tap itself (`pv_yuv_views`): no RGB
    copy is made, and a pitched decoder surface is read in place.  Classification models only.  The layouts of
    `YUV16_LAYOUTS` ("P010" / "P012" / "P016" / "I010" / "I012" / "I016": uint16 or int16 tensors, what a decoder hands out
    for 10- to 16-bit streams) go through every one of these paths the same way (`pv_yuv16_views`, `PV_U16`); a
    (standard, full_range) pair is composed with the layout's depth and bit alignment, and no narrowing pass exists.
    `hdr` -- "pq", "hlg" or (transfer, `tone_params(...)`), for a layout of `YUV16_LAYOUTS` only (a ValueError otherwise) --
    maps every tap from BT.2020 PQ / HLG to BT.709 SDR before the blend: every path of such a packer launches `pv_hdr_views`.

    `src_layout` of `PACKED_LAYOUTS` ("BGR", "RGBA", "BGRA", "ARGB", "ABGR"; "RGBX" / "BGRX" / "XRGB" / "XBGR" are aliases):
    uint8 packed pixels, [B, T, H, W, PB] clips, [N, H, W, PB] videos or `FrameList`s of [H, W, PB] frames, with
    stride(-1) == 1, stride(-2) == PB and a row stride >= W * PB (`packed_geometry`; a ValueError names the stride otherwise,
    and nothing is ever made contiguous): OpenCV's BGR24 and pitched 32-bit capture / compositor surfaces are read where they
    lie, the tensor's row and frame strides being the record's y_pitch / frame_stride.  Every path of such a packer is
    item-sourced (`pv_batch_views`, `pv_frame_views`, `pv_region_views`, `pv_area_views`: the clip-at-a-time call and
    `fill_video` run a batch with every clip, or the one video, a source of its own), `keyframes=True`, `regions=True`,
    `interpolation="area"` and `orientation=` included; `hdr` is refused, as for every layout without 16-bit samples.  An item
    holds the bits of the "NTHWC" path on `packed_to_rgb(video, layout).contiguous()`.

    `fill_video(video, tables, i0, n)` + `launch()` run the resampling packer on ONE decoded video instead of clips: items
    [i0, i0 + n) of its clips x views sequence, the clips being rows of a frame table (`data.clip_frame_table`, uploaded by
    `video_tables`) that the ingest kernel reads the video through (`pv_video_views`); `inference.VideoPredictor` is the
    loop around it.

    `video_batch(videos, tables)` + `fill_batch(batch, i0, n)` + `launch()` do the same for MANY videos of any lengths and
    frame sizes at once: every item of the deploy batch has a source of its own (`pv_batch_views`), so a forward is filled
    with views of as many videos as it takes; `inference.VideoBatchPredictor` is the loop around it.

    `keyframes=True` with `short_side` and WITHOUT `crop_size`: no crop -- the window is the whole scaled frame, which must be the deploy form's H x W
    (rectangular for a rectangular source: 256 x 455 for 720p); this mode runs through `video_batch` / `fill_batch` only.
    `keyframes=True` in general makes the packer the ingest of key-frame detection: `video_batch` / `fill_batch` accept a detection form
    (one view; every item is the clip around one key frame), any source layout is legal -- the boxes no longer pass through
    the host -- and `fill_boxes(batch, boxes_dev, box_item_dev, box0, n, item0, n_items)` fills the form's box buffer for the
    forward `fill_batch(batch, item0, n_items)` filled (`pv_box_views`); `inference.KeyframeDetector` is the loop around it.
    The clip-at-a-time `packer(clip, bboxes)` keeps mapping the boxes on the host and keeps refusing YUV clips.

    `regions=True` with `crop_size` (an int or (Ho, Wo): the deploy form's H x W) and WITHOUT `short_side` makes the packer the
    ingest of actor tubes: `video_batch(videos, tables, regions=[...])` takes a rectangle (top, left, h, w) per frame of
    every table row, and `fill_batch` resizes each rectangle of the video, read where it lies, to `crop_size`
    (`pv_region_views`) -- no short-side scale, no crop window, one view; classification forms, any source layout, whole
    videos or `FrameList`s; no `orientation` and no `hdr`.  This mode runs through `video_batch` / `fill_batch` only;
    `inference.TubePredictor` is the loop around it.

    `interpolation="area"` scales with a box filter -- `short_side_scale(x, size, "area")`, every source pixel under an output
    pixel averaged, what a 720p or larger source needs -- instead of four taps: `video_batch` / `fill_batch` then launch
    `pv_area_views`, for whole videos and `FrameList`s, every source layout, `keyframes=True` and its no-crop mode included
    (boxes depend on the geometry only: `fill_boxes` is the same).  A ValueError with `regions=True`, with `hdr`, for a
    non-zero `orientation` in `video_batch` and for the clip-at-a-time `packer(clip)` call (use `video_batch` or
    `device_scale_crop`)."""

    def __init__(self, deployed, mean=None, std=None, div255=False, frame_ratios=None, short_side=None, crop_size=None,
                 spatial_idx=1, src_layout="NCTHW", yuv=("bt709", False), coded_height=None, height=None, keyframes=False,
                 hdr=None, regions=False, interpolation="bilinear"):
        self.subs = None
        self.region_mode = bool(regions)
        self.area = _interpolation(interpolation, None, hdr, "DevicePacker")
        if self.area and self.region_mode:
            raise ValueError("interpolation='area' is not supported together with regions: pv_region_views resizes a tube by "
                             "about 1-2x with four taps")
        if self.area and short_side is None:
            raise ValueError("interpolation='area' is the filter of the short-side scale: give short_side")
        if self.region_mode:
            # the ingest of actor tubes: no short-side scale and no crop window -- every frame's rectangle is resized to crop_size
            if short_side is not None:
                raise ValueError("a regions packer resizes every rectangle to crop_size: short_side=%r contradicts it (the "
                                 "whole frame is not scaled); give crop_size alone" % (short_side,))
            if crop_size is None or keyframes:
                raise ValueError("a regions packer takes crop_size, an int or (Ho, Wo): the size every rectangle is resized to"
                                 " (keyframes=True is the detection models' path)")
            if hdr is not None:
                raise ValueError("hdr is not supported together with regions: pv_region_views has no PQ / HLG tap map")
            if _views(spatial_idx) != (1,):
                raise ValueError("a regions packer has one view (a rectangle is resized whole): spatial_idx=%r" % (spatial_idx,))
            if getattr(deployed, "_pv_load_boxes", None) is not None:
                raise ValueError("a detection model pools its boxes from the whole frame's features: inference.KeyframeDetector")
            crop_size = _size_pair(crop_size, "crop_size")
        elif (short_side is None) != (crop_size is None) and not (keyframes and crop_size is None):
            raise ValueError("short_side and crop_size are given together (short_side alone -- no crop -- is a mode of the "
                             "key-frame path: keyframes=True)")
        # keyframes=True and short_side alone: no crop (the detection tutorial's protocol) -- the window is the whole scaled frame
        self.no_crop, self.keyframes = short_side is not None and crop_size is None, bool(keyframes)
        if src_layout not in _SRC_LAYOUTS:
            raise ValueError(_LAYOUT_ERROR)
        self.short_side, self.crop_size, self.src_layout = short_side, crop_size, src_layout
        self.is_yuv, self.coded_height, self.height = src_layout in _YUV_ANY, coded_height, height
        self.is_yuv16 = src_layout in _YUV_WIDE                # 16-bit samples: pv_yuv16_views / PV_U16
        self.is_packed = src_layout in _PACKED_ANY             # packed pixels: item-sourced launches only
        self.is_yuv4 = src_layout in _YUV4_ANY                 # YUV 4:2:2 (planar or packed) / 4:4:4: item-sourced launches only
        self.video_dims = 1 + _yuv_dims(src_layout) if self.is_yuv else 4   # of one whole video in this layout
        self.item_only = self.is_packed or self.is_yuv4        # the one-source entry points do not read these
        self.region_even = region_evenness(src_layout)         # what `box_regions(..., even=)` takes for this layout
        self.in_place = self.is_yuv or self.is_packed          # read with the strides they have: never made contiguous
        self._items_video = None
        self.hdr = _hdr_of(hdr, src_layout)                    # (PV_TRANSFER code, tone table) or None; on the device below
        self._hdr_src = None
        if self.in_place and not self.keyframes and (getattr(deployed, "_pv_load_boxes", None) is not None):
            raise ValueError("a detection model does not take %s frames: its boxes are mapped through the scaling and the crop "
                             "of an RGB clip on the host, and that path is not built for YUV sources (the key-frame path, "
                             "keyframes=True / inference.KeyframeDetector, maps them on the device for any layout)" % src_layout)
        self.views = _views(spatial_idx) if crop_size is not None else (1,)
        if short_side is None and src_layout != "NCTHW" and not self.region_mode:
            raise ValueError("a frame-interleaved, packed or YUV clip is read by the resampling path only: give short_side and crop_size")
        if hasattr(deployed, "parts") and hasattr(deployed, "_pv_launch"):
            # split-batch deploy form (convert_to_deployable_form(..., streams=k)): one packer per sub-batch fills that
            # sub-plan's input buffers, then ONE launch of the joint graph
            self.model = deployed
            self.subs = [DevicePacker(p, mean, std, div255, frame_ratios, short_side, crop_size, spatial_idx, src_layout, yuv,
                                      coded_height, height, keyframes, hdr, regions, interpolation) for p in deployed.parts]
            self.window = self.subs[0].window
            self.sess, self.refs = self.subs[0].sess, self.subs[0].refs
            self.frame_ratios = self.subs[0].frame_ratios
            self._clip_tables = {}
            return
        inputs = getattr(deployed, "_pv_inputs", None)
        if inputs is None:
            raise RuntimeError("DevicePacker needs a model converted as a whole by convert_to_deployable_form(model, x)")
        self.model = deployed
        self.sess = deployed._pv_session
        self.refs = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
        if frame_ratios is None:
            if len(self.refs) != 1:
                raise ValueError("frame_ratios is required for a model with %d input pathways" % len(self.refs))
            frame_ratios = (1,)
        if len(frame_ratios) != len(self.refs):
            raise ValueError("%d frame ratios for %d input pathways" % (len(frame_ratios), len(self.refs)))
        self.frame_ratios = tuple(int(r) for r in frame_ratios)
        if crop_size is not None:
            for ref in self.refs:
                if (ref.H, ref.W) != (crop_size if self.region_mode else (crop_size, crop_size)):
                    raise ValueError("crop_size %s is not the %d x %d input the deploy form was converted for"
                                     % (crop_size, ref.H, ref.W))
            if len(self.views) > 1 and getattr(deployed, "_pv_load_boxes", None) is not None:
                raise ValueError("a detection model takes one view: its boxes belong to one crop")
        if any((ref.H, ref.W) != (self.refs[0].H, self.refs[0].W) for ref in self.refs):
            raise ValueError("the input pathways of one deploy form have one frame size")
        # (Ho, Wo) of the window every resampling launch writes: the crop, or -- no crop -- the deploy form's own H x W, which
        # every source must then scale to (checked per video, with both sizes named)
        self.window = (self.refs[0].H, self.refs[0].W) if crop_size is None or self.region_mode else (crop_size, crop_size)
        self.scale, self.shift = _affine(mean, std, div255, self.refs[0].C, self.sess.device)
        self._index = {}
        self._planar = {}
        self._clip_tables = {}
        self.yuv_matrix = _yuv_matrix_of(yuv, src_layout).float().reshape(12).to(self.sess.device) if self.is_yuv else None
        if self.hdr is not None:
            self.hdr = (self.hdr[0], self.hdr[1].to(self.sess.device))

    def _t_index(self, t_src, ref):
        key = (t_src, ref.T)
        if key not in self._index:
            idx = temporal_indices(t_src, ref.T)
            self._index[key] = None if (t_src == ref.T and torch.equal(idx, torch.arange(t_src))) \
                else idx.to(torch.int32).to(self.sess.device)
        return self._index[key]

    def _check_source(self, clip, want):
        """Everything that can be wrong with a clip for the resampling path, BEFORE any launch."""
        b, c, t, hs, ws = _source_geometry(clip, self.src_layout)
        if b * len(self.views) != want:
            raise RuntimeError("deploy form was converted for a batch of %d = clips x views, got %d clips x %d views"
                               % (want, b, len(self.views)))
        hn, wn, _ = _view_geometry(hs, ws, self.short_side, self.crop_size, self.views)
        if self.src_layout == "NTHWC" and (c != 3 or clip.dtype != torch.uint8):
            raise RuntimeError("a frame-interleaved clip is uint8 [B,T,H,W,3], got %s %s" % (clip.dtype, tuple(clip.shape)))
        for ratio, ref in zip(self.frame_ratios, self.subs[0].refs if self.subs is not None else self.refs):
            if c != ref.C or t // ratio != ref.T:
                raise RuntimeError("pathway with frame ratio %d expects %d channels x %d frames, the clip gives %d x %d"
                                   % (ratio, ref.C, ref.T, c, t // ratio))
        return hs, ws, hn, wn

    def _boxes_to_crop(self, bboxes, hs, ws, hn, wn):
        """[R,5] boxes (batch index, x1, y1, x2, y2 in source pixels) -> the same in the pixels of the crop."""
        out = bboxes.detach().to("cpu", torch.float32).clone()
        out[:, 1:5] *= float(hn) / hs if ws < hs else float(wn) / ws        # short_side_scale_with_boxes
        y, x = crop_offsets(hn, wn, self.crop_size, self.views[0])
        out[:, 1:5] = clip_boxes_to_image(crop_boxes(out[:, 1:5], x, y), self.crop_size, self.crop_size)
        return out

    @torch.no_grad()
    def __call__(self, clip, bboxes=None, orientation=0):
        if self.area:
            raise ValueError("interpolation='area' runs through video_batch / fill_batch (every item a source of its own: "
                             "pv_area_views); for clips alone use device_scale_crop(..., interpolation='area')")
        _refuse_orientation(orientation, "a clip-at-a-time call")
        if self.region_mode:
            raise RuntimeError("a regions packer runs through video_batch(..., regions=) / fill_batch; clips with a rectangle "
                               "per frame alone: device_resized_crop")
        load_boxes = getattr(self.model, "_pv_load_boxes", None)
        if (bboxes is None) != (load_boxes is None):
            raise RuntimeError("bboxes are given to a detection model and only to a detection model")
        if self.in_place and load_boxes is not None:
            raise ValueError("a detection model does not take %s frames a clip at a time: its boxes are mapped on the host "
                             "there; use video_batch / fill_batch / fill_boxes (inference.KeyframeDetector)" % self.src_layout)
        _refuse_frames(clip, "a clip-at-a-time call")
        if self.no_crop:
            raise RuntimeError("the no-crop mode (short_side without crop_size) runs through video_batch / fill_batch / "
                               "fill_boxes; a clip at a time takes short_side and crop_size")
        if self.item_only:
            return self._call_items(clip)
        if self.is_yuv:
            return self._call_yuv(clip)
        if clip.dim() != 5:
            raise RuntimeError("expected a [B,C,T,H,W] clip, got %s" % (tuple(clip.shape),))
        resample = self.short_side is not None
        if self.subs is not None:
            # validate BEFORE any ingest: a short batch must not reach the sub-plans' input buffers
            want = sum(self.model._splits)
            if resample:
                self._check_source(clip, want)
            elif clip.shape[0] != want:
                raise RuntimeError("deploy form was converted for a batch of %d, got %d" % (want, clip.shape[0]))
            if bboxes is not None:
                raise RuntimeError("bboxes cannot be given to a split-batch deploy form (detection models are converted as one plan)")
            clip = _device_source(clip, self.sess.device) if resample else clip.to(self.sess.device, non_blocking=True)
            lo = 0
            for sub, b in zip(self.subs, self.model._splits):
                if resample:
                    sub._fill_resampled(clip, lo, b)      # destination items [lo, lo + b) of the clips x views sequence
                else:
                    sub._fill(clip[lo:lo + b])
                lo += b
            return self.launch()
        if resample:
            hs, ws, hn, wn = self._check_source(clip, self.refs[0].B)
            if bboxes is not None:
                bboxes = self._boxes_to_crop(bboxes, hs, ws, hn, wn)
            self._fill_resampled(_device_source(clip, self.sess.device), 0, self.refs[0].B)
        else:
            clip = clip.to(self.sess.device, non_blocking=True)
            self._fill(clip)
        if load_boxes is not None:
            load_boxes(bboxes)
        return self.launch()

    def _call_yuv(self, clips):
        """B materialised YUV clips [B, T', Hc*3/2, W]: the sequence of B * T' frames read through a table whose row b is
        b * T' + the frames every pathway subsamples -- `fill_video` on that table, then the forward."""
        if clips.dim() != 4:
            raise RuntimeError("expected %s clips [B, T, Hc*3/2, W], got %s" % (self.src_layout, tuple(clips.shape),))
        b, t = clips.shape[:2]
        if b * len(self.views) != self.batch:
            raise RuntimeError("deploy form was converted for a batch of %d = clips x views, got %d clips x %d views"
                               % (self.batch, b, len(self.views)))
        refs = self.subs[0].refs if self.subs is not None else self.refs
        for ratio, ref in zip(self.frame_ratios, refs):
            if t // ratio != ref.T:
                raise RuntimeError("pathway with frame ratio %d expects %d frames, the clip gives %d" % (ratio, ref.T, t // ratio))
        if (b, t) not in self._clip_tables:
            self._clip_tables[(b, t)] = [_clip_rows(b, t, ref.T).to(self.sess.device) for ref in refs]
        self.fill_video(clips.to(self.sess.device, non_blocking=True), self._clip_tables[(b, t)], 0, self.batch)
        return self.launch()

    def _call_items(self, clips):
        """B materialised clips of packed pixels [B, T', H, W, PB] -- or of YUV 4:2:2 / 4:4:4 frames [B, T', rows, W] --, read
        with the strides they have: every clip a source of its own, its frames one table row (`video_batch` + `fill_batch`:
        pv_batch_views), then the forward."""
        if self.is_yuv4 and clips.dim() != 1 + self.video_dims:
            raise RuntimeError("expected %s clips [B, T, %s], got %s" % (self.src_layout, "H, W, 2" if self.video_dims == 4 else "rows, W", tuple(clips.shape),))
        if self.is_packed and clips.dim() != 5:
            raise RuntimeError("expected %s clips [B, T, H, W, %d], got %s" % (self.src_layout, _packed_bytes(self.src_layout), tuple(clips.shape),))
        b, t = clips.shape[:2]
        if b * len(self.views) != self.batch:
            raise RuntimeError("deploy form was converted for a batch of %d = clips x views, got %d clips x %d views"
                               % (self.batch, b, len(self.views)))
        if t != self.clip_frames:
            raise RuntimeError("the deploy form takes clips of %d frames, the clips have %d" % (self.clip_frames, t))
        rows = torch.arange(t, dtype=torch.int32)[None]
        batch = self.video_batch(list(clips.to(self.sess.device, non_blocking=True).unbind(0)), [rows] * b)
        self.fill_batch(batch, 0, batch.total)
        return self.launch()

    def _fill_items_video(self, video, tables, i0, n):
        """`fill_video` of packed pixels and of YUV 4:2:2 / 4:4:4: the one-source entry points do not read them, so the video
        is a batch of one (pv_batch_views) whose records and items are uploaded once per (video, tables) and whose frame
        tables are the caller's, already on the device."""
        key = (video.data_ptr(), tuple(video.shape), video.stride(), tuple(t.data_ptr() for t in tables))
        if self._items_video is None or self._items_video[0] != key:
            rows = torch.zeros((tables[0].shape[0], self.clip_frames), dtype=torch.int32)   # frame 0: the tables are the caller's
            batch = self.video_batch([video], [rows])
            batch.tables = list(tables)
            self._items_video = (key, batch)
        self.fill_batch(self._items_video[1], i0, n)

    def _fill(self, clip):
        t_src = clip.shape[2]
        for ratio, ref in zip(self.frame_ratios, self.refs):
            if t_src // ratio != ref.T:
                raise RuntimeError("pathway with frame ratio %d expects %d frames, the clip gives %d" % (ratio, ref.T, t_src // ratio))
            self.sess.ingest(clip, ref, t_index=self._t_index(t_src, ref), ch_scale=self.scale, ch_shift=self.shift)

    def _fill_resampled(self, clip, item0, n_items):
        """One pv_resample_crop launch per pathway: items [item0, item0 + n_items) of the clips x views sequence."""
        from . import _lib as L
        self._src = clip                                   # alive until the launch has run
        for i, ref in enumerate(self.refs):
            d = _resample_desc(clip, self.src_layout, self.short_side, self.crop_size, self.views)
            d.item0, d.n_items = item0, n_items
            index = self._t_index(d.src_T, ref)
            if index is not None:
                d.T, d.t_index = ref.T, index.data_ptr()
            _set_affine(d, self.scale, self.shift)
            self.sess.resample(d, ref, planar=self._planar_for(i, ref))

    def _planar_for(self, i, ref):
        """The packer's own bf16 NCDHW clip for pathway i when every reader of `ref` is a stem that reads such a clip itself
        (the resampling kernels write it and the stem is pointed there), else None: the arena buffer in its own layout."""
        from . import _lib as L
        if ref.src_slot is None or ref.c4_readers != 0 or self.sess.pv_dtype != L.PV_BF16:
            return None
        if i not in self._planar:
            self._planar[i] = torch.empty((ref.B, ref.C, ref.T, ref.H, ref.W), dtype=torch.bfloat16, device=self.sess.device)
        return self._planar[i]

    # ------------------------------------------------------------------------- whole-video ingest (pv_video_views)
    @property
    def batch(self):
        """Items of one forward of the deploy form (clips x views)."""
        return sum(self.model._splits) if self.subs is not None else self.refs[0].B

    @property
    def clip_frames(self):
        """Frames of the clip the pathways subsample (SlowFast (4, 1): the fast pathway's)."""
        refs = self.subs[0].refs if self.subs is not None else self.refs
        t = max(ref.T * r for ref, r in zip(refs, self.frame_ratios))
        if any(t // r != ref.T for ref, r in zip(refs, self.frame_ratios)):
            raise ValueError("frame ratios %s do not fit the pathways' frame counts %s" % (self.frame_ratios, [ref.T for ref in refs]))
        return t

    def video_tables(self, table, num_frames):
        """Upload (once per video) the per-pathway frame tables of a [n_clips, clip_frames] table: `pathway_tables`."""
        refs = self.subs[0].refs if self.subs is not None else self.refs
        table = torch.as_tensor(table)
        if table.dim() == 2 and table.shape[1] != self.clip_frames:
            raise ValueError("the deploy form takes clips of %d frames, the table has %d columns" % (self.clip_frames, table.shape[1]))
        return [t.to(self.sess.device) for t in pathway_tables(table, [ref.T for ref in refs], num_frames)]

    @torch.no_grad()
    def fill_video(self, video, tables, i0, n):
        """Fill the deploy form's input buffers with items [i0, i0 + n) of the clips x views sequence of ONE video (item
        clip * n_views + v is view v of the clip whose frames are row `clip` of `tables`, from `video_tables`), one
        pv_video_views launch per pathway (and per sub-plan of a split-batch form): no clip is materialised.  n may be
        smaller than the deploy batch -- the ragged last chunk of a video -- and the rest of the buffers is then zeroed.
        `video` is [C,N,H,W] ("NCTHW"; uint8 or fp32) or [N,H,W,3] uint8 ("NTHWC"), contiguous and on the device -- or, for a
        YUV layout, uint8 [N, Hc*3/2, W] on the device with the strides it has (`yuv_geometry`) -- and must stay alive until
        the forward has run.  Nothing is launched here but the ingest: run `launch()` next."""
        _refuse_frames(video, "fill_video")
        if self.area:
            raise ValueError("interpolation='area' runs through video_batch / fill_batch (pv_area_views), a video alone as a "
                             "batch of one")
        if self.short_side is None or self.no_crop:
            raise RuntimeError("fill_video resamples: construct the packer with short_side and crop_size")
        if getattr(self.model, "_pv_load_boxes", None) is not None:
            raise RuntimeError("a detection model takes boxes of key frames, not a video")
        c, nf, hs, ws, geom = _video_source(video, self.src_layout, torch.device(self.sess.device), self.coded_height, self.height)
        source = (c, nf, hs, ws, geom, _view_geometry(hs, ws, self.short_side, self.crop_size, self.views))
        refs = self.subs[0].refs if self.subs is not None else self.refs
        if len(tables) != len(refs):
            raise RuntimeError("%d frame tables for %d input pathways" % (len(tables), len(refs)))
        for tab, ref in zip(tables, refs):
            if (tab.dim() != 2 or tab.dtype != torch.int32 or not tab.is_cuda or not tab.is_contiguous()
                    or tab.shape[0] != tables[0].shape[0] or tab.shape[1] != ref.T or c != ref.C):
                raise RuntimeError("pathway expects %d channels and an int32 device table [n_clips, %d]; got %d channels, %s %s"
                                   % (ref.C, ref.T, c, tab.dtype, tuple(tab.shape)))
        total = tables[0].shape[0] * len(self.views)
        if not (0 <= i0 and 0 < n <= self.batch and i0 + n <= total):
            raise RuntimeError("items [%d, %d) are not a chunk of at most %d of the video's %d clips x views"
                               % (i0, i0 + n, self.batch, total))
        if self.item_only:
            return self._fill_items_video(video, tables, i0, n)
        if self.subs is None:
            return self._fill_video(video, source, tables, i0, n)
        lo = 0
        for sub, b in zip(self.subs, self.model._splits):
            sub._fill_video(video, source, tables, i0 + lo, max(0, min(b, n - lo)))
            lo += b

    def launch(self):
        """One forward on what the input buffers hold; the logits [batch, classes] (an arena view for a one-plan form:
        valid until the next forward)."""
        if self.subs is not None:
            self.model._pv_launch()
        else:
            self.sess.launch(use_graph=self.model._pv_use_graph)
        return self.model._pv_result()

    def _fill_video(self, video, source, tables, item0, n_items):
        """One pv_video_views (YUV: pv_yuv_views / pv_yuv16_views) launch per pathway into this plan's buffers; `source` is
        what `fill_video` found out about the video: `_video_source` and `_view_geometry`.  See Session.video_views for the
        tail."""
        from . import _lib as L
        self._src = (video, tables)                        # alive until the launch has run
        c, nf, hs, ws, geom, geo = source
        if self.hdr is not None:
            # pv_yuv16_views has no tap map: the video is the one record of pv_hdr_views launches, uploaded once per video
            if self._hdr_src is None or self._hdr_src.key != HdrVideoSource.key_of(video, geom, geo, tables[0].shape[0], len(self.views)):
                self._hdr_src = HdrVideoSource(video, geom, geo, tables[0].shape[0], len(self.views), self.sess.device)
            for i, (ref, tab) in enumerate(zip(self.refs, tables)):
                h = self._hdr_src.desc(tab, self.yuv_matrix, self.src_layout, self.window, self.hdr, item0, n_items)
                _set_affine(h.frames.batch, self.scale, self.shift)
                self.sess.hdr_views(h, ref, planar=self._planar_for(i, ref))
            return
        for i, (ref, tab) in enumerate(zip(self.refs, tables)):
            if self.is_yuv:
                d = _yuv_desc(video, geom, tab, self.yuv_matrix, self.short_side, self.crop_size, self.views, geo)
                fill = self.sess.yuv16_views if self.is_yuv16 else self.sess.yuv_views
            else:
                d = _rgb_source(L.VideoViewsDesc(), video, self.src_layout, c, hs, ws, geo, self.crop_size)
                d.t_index, d.n_clips, d.T, d.N, d.t_stride = tab.data_ptr(), tab.shape[0], ref.T, nf, tab.stride(0)
                fill = self.sess.video_views
            d.item0, d.n_items = (item0, n_items) if n_items else (0, 0)
            _set_affine(d, self.scale, self.shift)
            fill(d, ref, planar=self._planar_for(i, ref))

    # ------------------------------------------------------------------------- many videos per forward (pv_batch_views)
    def video_batch(self, videos, tables, height=None, coded_height=None, orientation=None, regions=None):
        """Prepare a list of decoded videos -- any lengths, any frame sizes, all in the packer's source layout and on the
        device -- for `fill_batch`: `tables[j]` is the [n_clips_j, clip_frames] frame table of video j
        (`data.clip_frame_table`).  Every video is validated as `fill_video` validates one (device, dtype, contiguity of the
        RGB / planar forms, `yuv_geometry` of the YUV forms with `height` / `coded_height` as one number or one per video,
        the crop fits the scaled frame, every table entry names a frame of ITS video), then the per-video records, the
        video-major item sequence (video j, then clip * n_views + v) and the concatenated per-pathway tables are uploaded
        ONCE.  The videos may instead ALL be `FrameList`s -- one device tensor per frame, as a decoder's surface pool hands
        them out: one table of frame addresses is then uploaded with the records, and `fill_batch` reads every frame where
        it lies (`pv_frame_views`); a mix of tensors and FrameLists is a ValueError.  `orientation`: one code
        (`orientation_code`) or one per video for videos STORED turned and / or mirrored -- a portrait phone clip is landscape
        frames plus "rotate 90": the ingest reads them in place and cuts the views from the displayed frame, and
        `fill_boxes` takes boxes given in stored pixels along.  Returns a `VideoBatch`, which keeps the videos alive.
        `regions` (a packer constructed with `regions=True` and `crop_size` alone, and only such a packer): one integer
        tensor [n_clips_j, clip_frames, 4] of (top, left, h, w) per video, aligned with `tables[j]` -- destination frame t of
        row r is the rectangle `regions[j][r, t]` of frame `tables[j][r, t]`, resized to `crop_size` (`pv_region_views`; `box_regions` makes
        rectangles of boxes).  Validated here (inside the frame, at least 1 x 1, even members for YUV layouts) and uploaded
        once, with the records.  ValueError together with `orientation`; such a packer has no `hdr` and one view."""
        if self.area:
            _interpolation("area", orientation, None, "video_batch")
        if self.region_mode != (regions is not None):
            if regions is not None:
                raise ValueError("regions are resized to crop_size with no short-side scale: this packer scales every frame by "
                                 "short_side=%r, which contradicts them -- construct it with regions=True and crop_size alone"
                                 % (self.short_side,))
            raise ValueError("a regions packer takes video_batch(videos, tables, regions=[...])")
        if self.short_side is None and not self.region_mode:
            raise RuntimeError("video_batch resamples: construct the packer with short_side and crop_size")
        if getattr(self.model, "_pv_load_boxes", None) is not None and not self.keyframes:
            raise RuntimeError("a detection model takes boxes of key frames, not videos: construct the packer with "
                               "keyframes=True and fill the boxes with fill_boxes (inference.KeyframeDetector)")
        refs = self.subs[0].refs if self.subs is not None else self.refs
        for t in tables:
            t = torch.as_tensor(t)
            if t.dim() == 2 and t.shape[1] != self.clip_frames:
                raise ValueError("the deploy form takes clips of %d frames, the table has %d columns" % (self.clip_frames, t.shape[1]))
        device = torch.device(self.sess.device)
        return build_video_batch(videos, tables, self.src_layout, self.short_side,
                                 self.window if self.no_crop else self.crop_size, self.views,
                                 [ref.T for ref in refs], refs[0].C, device, lambda t: t.to(device),
                                 self.height if height is None else height,
                                 self.coded_height if coded_height is None else coded_height, orientation, regions)

    @torch.no_grad()
    def fill_batch(self, batch, i0, n):
        """Fill the deploy form's input buffers with items [i0, i0 + n) of the sequence of `batch` (`video_batch`), n at most
        the deploy batch: one pv_batch_views launch per pathway (and per sub-plan of a split-batch form -- a sub-plan's window
        is a pointer offset into the item sequence).  A short chunk zeroes the rest of the buffers, as `fill_video` does.
        Nothing is launched here but the ingest: run `launch()` next."""
        if not isinstance(batch, VideoBatch) or batch.n_views != len(self.views) or (batch.regions is not None) != self.region_mode:
            raise RuntimeError("fill_batch takes what video_batch of this packer returned")
        if not (0 <= i0 and 0 < n <= self.batch and i0 + n <= batch.total):
            raise RuntimeError("items [%d, %d) are not a chunk of at most %d of the batch's %d items" % (i0, i0 + n, self.batch, batch.total))
        if self.subs is None:
            return self._fill_batch(batch, i0, n)
        lo = 0
        for sub, b in zip(self.subs, self.model._splits):
            sub._fill_batch(batch, i0 + lo, max(0, min(b, n - lo)))
            lo += b

    def release_batch(self):
        """Drop the packer's reference to the last `VideoBatch` (and with it to all its videos); call once the last forward
        on it has been launched.  Work already queued stays valid: the memory is reused in stream order."""
        for p in (self.subs if self.subs is not None else [self]):
            p._src = None
        self._boxes_src = None

    def _fill_batch(self, batch, item0, n_items):
        """One pv_batch_views launch per pathway into this plan's buffers -- pv_frame_views, the same descriptor with the
        call's pointer table beside it, for a batch of FrameLists; pv_region_views, with the pathway's rectangle table beside
        both, for a batch built with `regions=`; pv_area_views, the filter beside either source form, for a packer with
        `interpolation="area"`; see Session.video_views for the tail."""
        from . import _lib as L
        self._src = batch                                  # alive until the launch has run
        for i, (ref, tab) in enumerate(zip(self.refs, batch.tables)):
            g = L.RegionViewsDesc() if batch.regions is not None else None   # pv_region_views: either source form, rectangles behind
            h = L.HdrViewsDesc() if self.hdr is not None else None           # pv_hdr_views: either source form, tap map behind
            a = L.AreaViewsDesc() if self.area else None                     # pv_area_views: either source form, the filter behind
            f = (a.frames if a is not None else g.frames if g is not None else h.frames if h is not None
                 else (L.FrameViewsDesc() if batch.frame_ptrs is not None else None))
            d = L.BatchViewsDesc() if f is None else f.batch
            _batch_launch_fields(d, batch, tab, item0, n_items, ref.C, self.src_layout, self.yuv_matrix, self.window)
            _set_affine(d, self.scale, self.shift)
            if f is None:
                self.sess.batch_views(d, ref, planar=self._planar_for(i, ref))
                continue
            if batch.frame_ptrs is not None:
                f.frame_ptrs, f.frame_ptrs_dev = batch.frame_ptrs.data_ptr(), batch.frame_ptrs_dev.data_ptr()
                f.n_frame_ptrs = batch.frame_ptrs.numel()
            if a is not None:
                a.filter = L.PV_FILTER_AREA
                self.sess.area_views(a, ref, planar=self._planar_for(i, ref))
                continue
            if g is not None:
                g.regions, g.regions_dev = batch.regions[i].data_ptr(), batch.regions_dev[i].data_ptr()
                self.sess.region_views(g, ref, planar=self._planar_for(i, ref))
                continue
            if h is None:
                self.sess.frame_views(f, ref, planar=self._planar_for(i, ref))
                continue
            h.transfer, h.tone = self.hdr[0], self.hdr[1].data_ptr()
            self.sess.hdr_views(h, ref, planar=self._planar_for(i, ref))

    # ------------------------------------------------------------------------- key-frame detection (pv_box_views)
    @property
    def box_capacity(self):
        """Rows of the detection form's box buffer: the box count it was converted for."""
        cap = getattr(self.model, "_pv_box_capacity", None)
        if cap is None:
            raise RuntimeError("fill_boxes needs a detection model converted as a whole by convert_to_deployable_form")
        return cap

    @torch.no_grad()
    def fill_boxes(self, batch, boxes_dev, box_item_dev, box0, n, item0, n_items, clip_to_source=None, dst_box=None):
        """Fill the detection form's box buffer for the forward that `fill_batch(batch, item0, n_items)` filled: boxes
        [box0, box0 + n) of `boxes_dev` (fp32 [N,4] on the device, x1 y1 x2 y2 in the pixels of each key frame's SOURCE frame)
        are mapped into the view of their item -- `box_item_dev` (int32 [N], non-decreasing, on the device) names it by its
        position in the sequence of `batch` -- by ONE `pv_box_views` launch; rows [n, capacity) get clip index -1.  Both
        tensors are uploaded once per call, not per forward.  `clip_to_source` (default: the no-crop mode) clips the boxes to
        the source frame first, as the detection tutorial does.  `dst_box`: an int32 [capacity] device tensor that receives
        the box number of every row (-1 behind the n-th)."""
        import ctypes as C
        from . import _lib as L
        if self.subs is not None:
            raise RuntimeError("fill_boxes needs a one-plan detection form")
        cap = self.box_capacity
        if not isinstance(batch, VideoBatch) or batch.n_views != len(self.views):
            raise RuntimeError("fill_boxes takes what video_batch of this packer returned")
        for t, dt, shape in ((boxes_dev, torch.float32, (boxes_dev.shape[0], 4)), (box_item_dev, torch.int32, (boxes_dev.shape[0],))):
            if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("boxes are a contiguous fp32 [N,4] and box_item an int32 [N] tensor on the device; got %s %s"
                                   % (t.dtype, tuple(t.shape)))
        if dst_box is not None and (not dst_box.is_cuda or dst_box.dtype != torch.int32 or dst_box.numel() < cap
                                    or not dst_box.is_contiguous()):
            raise RuntimeError("dst_box is a contiguous int32 device tensor of at least %d entries" % cap)
        if not (0 <= box0 and 0 <= n <= cap and box0 + n <= boxes_dev.shape[0]):
            raise RuntimeError("boxes [%d, %d) are not a window of at most %d of the call's %d boxes" % (box0, box0 + n, cap, boxes_dev.shape[0]))
        if not (0 <= item0 and 0 < n_items <= self.batch and item0 + n_items <= batch.total):
            raise RuntimeError("items [%d, %d) are not a chunk of at most %d of the batch's %d items" % (item0, item0 + n_items, self.batch, batch.total))
        d = L.BoxViewsDesc()
        d.boxes, d.box_item = boxes_dev.data_ptr(), box_item_dev.data_ptr()
        d.sources_dev, d.items_dev = batch.sources_dev.data_ptr(), batch.items_dev.data_ptr()
        d.dst_box = dst_box.data_ptr() if dst_box is not None else None
        d.n_boxes, d.n_seq, d.n_sources, d.n_views = boxes_dev.shape[0], batch.total, len(batch.sources), len(self.views)
        d.box0, d.n_launch, d.item0, d.n_items = box0, n, item0, n_items
        d.Ho, d.Wo, d.capacity = self.window[0], self.window[1], cap
        d.clip_to_source = int(self.no_crop if clip_to_source is None else clip_to_source)
        self._boxes_src = (boxes_dev, box_item_dev, dst_box)       # alive until the launch has run
        self.sess.box_views(d, self.model._pv_box_ptr)
