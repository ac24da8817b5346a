"""Key-frame action detection over whole videos on the MI355X: `pv_box_views` against the host mirror bit for bit, rectangular
deploy forms of both detection builders, and `inference.KeyframeDetector` end to end against the oracle run per key frame on
clips built with the pinned host resampling (tests/spatial_util.py) and boxes mapped in the reference's order.

Score tolerances are the ones tests/test_roi_head.py uses and justifies: fp32 1e-3 absolute on sigmoid scores, bf16 2.5e-2."""
import ctypes as C
import json
import os

import pytest
import torch

import spatial_util as SU
import yuv_util as YU
from oracle import functional as OF
from oracle.weights import detection_fill, quantize_like_kernels, seeded_input
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.inference import KeyframeDetector, keyframe_chunks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FIX = json.load(open(os.path.join(GOLD, "keyframe_boxes.json")))
TOL = {torch.float32: 1e-3, torch.bfloat16: 2.5e-2}
KW = dict(mean=SU.MEAN, std=SU.STD, div255=True)
COUNTS = [2, 0, 3, 1, 4]
STAMPS = [0.4, 0.7, 1.0, 1.3, 1.6]
FPS, DURATION = 20, 0.8


def box_set(h, w):
    """The fixture's box set of an h x w frame (fp32 [13, 4])."""
    c = [c for c in FIX["cases"] if (c["height"], c["width"]) == (h, w) and c["crop_size"] is None][0]
    return torch.tensor(c["boxes"], dtype=torch.float32)


# ----------------------------------------------------------------------------- pv_box_views == the host mirror
def _expected_row(box, rec, view, short, ho, wo, clip):
    """One box through the mirrors in the reference's order, for the record's geometry and the launch's window."""
    b = box.view(1, 4).clone()
    if clip:
        b = TR.clip_boxes_to_image(b, rec.Hs, rec.Ws)
    _, b = TR.short_side_scale_with_boxes(torch.zeros(1, 1, rec.Hs, rec.Ws), b, short)
    return TR.clip_boxes_to_image(TR.crop_boxes(b, rec.x_off[view], rec.y_off[view]), ho, wo)[0]


def _box_batch(crop):
    """Three sources of different geometry; crop mode: three views, clips (2, 1, 1) -> 12 items (through build_video_batch);
    no-crop mode: one view, window origins 0, every source with its own scaled size."""
    sizes = [(60, 90), (90, 60), (53, 53)]
    videos = [torch.zeros(6, h, w, 3, dtype=torch.uint8, device="cuda") for h, w in sizes]
    tables = [torch.zeros(n, 4, dtype=torch.int32) for n in (2, 1, 1)]
    if crop is not None:
        return TR.build_video_batch(videos, tables, "NTHWC", 56, crop, (0, 1, 2), [4], 3, torch.device("cuda"), lambda t: t.cuda()), 56
    # no crop: build_video_batch insists on one scaled size per batch, the kernel does not -- square-crop records, windows moved to 0
    b = TR.build_video_batch(videos, tables, "NTHWC", 48, 48, (1,), [4], 3, torch.device("cuda"), lambda t: t.cuda())
    for rec in b.sources:
        rec.y_off[0] = rec.x_off[0] = 0
    b.sources_dev = torch.frombuffer(b.sources, dtype=torch.uint8).cuda()
    return b, 48


@pytest.mark.parametrize("crop", [48, None], ids=["crop", "no_crop"])
def test_box_views_kernel_equals_the_host_mirror(crop):
    from gpu_util import call
    batch, short = _box_batch(crop)
    ho, wo = (crop, crop) if crop is not None else (48, 72)
    clip = crop is None
    n_views = batch.n_views
    items = batch.item_rows                                       # [total, 4]: source, row, view, 0
    sets = [box_set(r.Hs, r.Ws) for r in batch.sources]
    boxes = torch.cat([sets[int(items[i, 0])].repeat(2, 1) for i in range(batch.total)])     # 26 boxes per item
    box_item = torch.arange(batch.total, dtype=torch.int32).repeat_interleave(26)
    n_boxes, capacity, extra = boxes.shape[0], 70, 3              # 70 rows: two workgroups of 64 threads, the second one partial
    boxes_d, item_d = boxes.cuda(), box_item.cuda()
    total = batch.total
    windows = [(0, 0, 0, total), (0, 1, 0, total), (0, capacity - 1, 0, total), (0, capacity, 0, total),      # n_launch
               (n_boxes - 30, 30, 0, total),
               (10, capacity, 1, 2),                                # item0 > 0, box0 > 0, boxes of items before and behind
               (26, 20, 1, 1)]
    for box0, n, item0, n_items in windows:
        dst = torch.full((capacity + extra, 5), 7.0, device="cuda")
        dst_box = torch.full((capacity + extra,), 77, dtype=torch.int32, device="cuda")
        d = L.BoxViewsDesc()
        d.boxes, d.box_item, d.dst, d.dst_box = boxes_d.data_ptr(), item_d.data_ptr(), dst.data_ptr(), dst_box.data_ptr()
        d.sources_dev, d.items_dev = batch.sources_dev.data_ptr(), batch.items_dev.data_ptr()
        d.n_boxes, d.n_seq, d.n_sources, d.n_views = n_boxes, total, len(batch.sources), n_views
        d.box0, d.n_launch, d.item0, d.n_items = box0, n, item0, n_items
        d.Ho, d.Wo, d.capacity, d.clip_to_source = ho, wo, capacity, int(clip)
        call("pv_box_views", d)
        want = torch.zeros(capacity + extra, 5)
        want[:, 0] = -1
        want[capacity:] = 7.0
        want_box = torch.full((capacity + extra,), -1, dtype=torch.int32)
        want_box[capacity:] = 77
        outside = 0
        for i in range(n):
            g = box0 + i
            want_box[i] = g
            rel = int(box_item[g]) - item0
            if not 0 <= rel < n_items:
                outside += 1
                continue
            src, _, view, _ = items[item0 + rel].tolist()
            rec = batch.sources[src]
            want[i, 0] = rel
            want[i, 1:] = _expected_row(boxes[g], rec, view, short, ho, wo, clip)
            if crop is not None or (rec.Hn, rec.Wn) == (ho, wo):       # where the public mirror applies, it is the same
                views = (0, 1, 2) if crop is not None else (1,)
                assert torch.equal(want[i, 1:], TR.boxes_to_view(boxes[g].view(1, 4), rec.Hs, rec.Ws, short, crop, views[view], clip)[0])
        what = "window %s" % ((box0, n, item0, n_items),)
        assert torch.equal(dst.cpu(), want), what                 # all five columns, the tail and the sentinel rows
        assert torch.equal(dst_box.cpu(), want_box), what
        if (box0, item0) == (10, 1):
            assert outside > 0 and outside < n                    # the window really cut boxes off on both sides
    # dst_box is optional
    dst = torch.full((capacity, 5), 7.0, device="cuda")
    d.dst, d.dst_box, d.box0, d.n_launch, d.item0, d.n_items = dst.data_ptr(), None, 0, 3, 0, total
    call("pv_box_views", d)
    assert torch.equal(dst[3:].cpu(), torch.tensor([-1.0, 0, 0, 0, 0]).repeat(capacity - 3, 1)) and bool((dst[:3, 0] == 0).all())


# ----------------------------------------------------------------------------- models
def _model(name):
    from pytorchvideo_amd.models import create_resnet_with_roi_head, create_slowfast_with_roi_head
    g = torch.load(os.path.join(GOLD, name + ".pt"), weights_only=False)
    factory = create_slowfast_with_roi_head if "slowfast" in name else create_resnet_with_roi_head
    m = detection_fill(factory(**g["cfg"]), g["seed"]).eval()
    return g, m


def _scores(name, g, sd, x, boxes):
    if "slowfast" in name:
        return OF.slowfast_detection_forward(sd, x[0], x[1], boxes, head_pool_kernels=g["cfg"]["head_pool_kernel_sizes"])
    return OF.resnet_detection_forward(sd, x, boxes)


def _input(name, seed, h, w, batch=2):
    if "slowfast" in name:
        fast = seeded_input((batch, 3, 16, h, w), seed)
        return [fast[:, :, TR.temporal_indices(16, 4)].clone(), fast]
    return seeded_input((batch, 3, 4, h, w), seed)


RECT_BOXES = torch.tensor([[0, 4.0, 6.0, 40.0, 30.0], [1, 0.0, 0.0, 71.0, 47.0], [1, -20.0, -30.0, 30.0, 20.0],
                           [0, 50.0, 20.0, 71.0, 47.0], [1, 30.0, 30.0, 30.5, 30.2]])
_FORMS = {}


def _form(name, dtype, h, w):
    """(deploy form, state dict the oracle uses for it, golden, conversion input), converted once per module run."""
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    key = (name, dtype, h, w)
    if key not in _FORMS:
        g, m = _model(name)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        if dtype == torch.bfloat16:
            sd = quantize_like_kernels(sd)
        x = _input(name, g["seed"], h, w)
        transmute_model(m, "mi355x")
        xd = [t.cuda().to(dtype) for t in x] if isinstance(x, list) else x.cuda().to(dtype)
        boxes = RECT_BOXES.clone()
        boxes[:, 1:] = boxes[:, 1:].clamp(max=min(h, w) - 1.0) if (h, w) != (48, 72) else boxes[:, 1:]
        dm = convert_to_deployable_form(m, (xd, boxes), dtype=dtype)
        _FORMS[key] = (dm, sd, g, x, xd, boxes)
    return _FORMS[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["resnet_det_r50_small", "slowfast_det_r50_small"])
def test_rectangular_deploy_forms_match_the_oracle(name, dtype):
    dm, sd, g, x, xd, boxes = _form(name, dtype, 48, 72)
    xo = x
    if dtype == torch.bfloat16:
        xo = [t.bfloat16().float() for t in x] if isinstance(x, list) else x.bfloat16().float()
    want = _scores(name, g, sd, xo, boxes)
    assert want.std().item() > 0.2 and 0.0 < want.min().item() and want.max().item() < 1.0      # not saturated
    got = dm(list(xd) if isinstance(xd, list) else xd, boxes)
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    err = (got.cpu() - want).abs().max().item()
    print("%s %s 48x72: worst score error %.3e (bound %.1e)" % (name, dtype, err, TOL[dtype]))
    assert err <= TOL[dtype], "score error %.3e" % err
    assert dm._pv_box_capacity == 5


# ----------------------------------------------------------------------------- end to end
def _video(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _oracle_rows(name, g, sd, dtype, rgb, fps, stamps, box_list, short, crop, view):
    """The oracle run per key frame: `rgb` is fp32 [N, 3, Hs, Ws] raw values; the clip is built with the pinned resampling,
    the boxes mapped in the reference's order (clip to the source first where nothing is cropped)."""
    n, _, hs, ws = rgb.shape
    frames = 16 if "slowfast" in name else 4
    table, _ = D.keyframe_frame_table(stamps, DURATION, n, fps, frames)
    hn, wn = TR.scaled_size(hs, ws, short)
    (y0, x0), (ho, wo) = ((0, 0), (hn, wn)) if crop is None else (TR.crop_offsets(hn, wn, crop, view), (crop, crop))
    scale, shift = SU.affine()
    rows = []
    for k, b in enumerate(box_list):
        if b.shape[0] == 0:
            continue
        clip = rgb[table[k].long()].permute(1, 0, 2, 3)                               # [3, T, Hs, Ws]
        x = SU.pinned_resample(clip, hn, wn, y0, x0, ho, wo, scale, shift)[None]
        if dtype == torch.bfloat16:
            x = x.bfloat16().float()
        mapped = TR.boxes_to_view(b, hs, ws, short, crop, view, clip_to_source=crop is None)
        bb = torch.cat([torch.zeros(b.shape[0], 1), mapped], 1)
        xin = [x[:, :, TR.temporal_indices(16, 4)], x] if "slowfast" in name else x
        rows.append(_scores(name, g, sd, xin, bb))
    return torch.cat(rows)


def _split(boxes, counts):
    out, i = [], 0
    for c in counts:
        out.append(boxes[i:i + c].clone())
        i += c
    return out


def _check(got, want, dtype, what):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32, what
    err = (got.cpu() - want).abs().max().item()
    print("%s: worst score error %.3e (bound %.1e)" % (what, err, TOL[dtype]))
    assert err <= TOL[dtype], "%s: score error %.3e" % (what, err)
    # most rows are different answers (two boxes of the set coincide once clipped), so a row out of place would show
    apart = (want[:, None] - want[None]).abs().amax(-1)[~torch.eye(want.shape[0], dtype=torch.bool)]
    assert (apart > 4 * TOL[torch.float32]).float().mean().item() > 0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["no_crop", "crop"])
@pytest.mark.parametrize("name", ["resnet_det_r50_small", "slowfast_det_r50_small"])
def test_keyframe_detector_matches_the_oracle_per_key_frame(name, mode, dtype):
    short, crop, view = (48, None, 1) if mode == "no_crop" else (56, 48, 2)
    dm, sd, g, _, _, _ = _form(name, dtype, 48, 72 if crop is None else 48)
    video = _video(40, 60, 90, 4100)
    box_list = _split(box_set(60, 90), COUNTS)
    ratios = (4, 1) if "slowfast" in name else None
    det = KeyframeDetector(dm, DURATION, short_side=short, crop_size=crop, spatial_idx=view, frame_ratios=ratios, **KW)
    got = det(video.cuda(), FPS, STAMPS, [b.cuda() if k % 2 else b for k, b in enumerate(box_list)])   # host or device boxes
    want = _oracle_rows(name, g, sd, dtype, video.permute(0, 3, 1, 2).float(), FPS, STAMPS, box_list, short, crop, view)
    assert tuple(got.shape) == (sum(COUNTS), 16)
    _check(got, want, dtype, "%s %s %s" % (name, mode, dtype))
    chunks = keyframe_chunks(COUNTS, 2, 5)
    assert det.forwards == len(chunks) == 2 and det.chunks == chunks == [[0, 2], [3, 4]]
    # a second call on the same detector gives the same rows (nothing of the first call is left in the buffers)
    again = det(video.cuda(), FPS, STAMPS[3:], box_list[3:])
    assert torch.equal(again, got[5:]) and det.forwards == 1
    with pytest.raises(ValueError, match="6 boxes"):
        det(video.cuda(), FPS, STAMPS[:1], [box_set(60, 90)[:6]])


def test_keyframe_detector_reads_nv12_frames():
    name, dtype = "resnet_det_r50_small", torch.bfloat16
    dm, sd, g, _, _, _ = _form(name, dtype, 48, 72)
    y, u, v = YU.planes(40, 60, 90, 4200)
    packed = YU.pack(y, u, v, "NV12")
    frames = packed.frames("cuda")
    box_list = _split(box_set(60, 90), COUNTS)
    det = KeyframeDetector(dm, DURATION, short_side=48, src_layout="NV12", yuv=("bt709", False), **KW)
    got = det(frames, FPS, STAMPS, box_list)
    rgb = TR.yuv420_to_rgb(packed.frames(), "NV12", TR.yuv_matrix("bt709", False).float())    # the pinned YUV mirror
    want = _oracle_rows(name, g, sd, dtype, rgb, FPS, STAMPS, box_list, 48, None, 1)
    _check(got, want, dtype, "NV12 no_crop bf16")
    assert det.forwards == 2


def test_keyframe_detector_scores_two_videos_in_one_call():
    name, dtype = "resnet_det_r50_small", torch.float32
    dm, sd, g, _, _, _ = _form(name, dtype, 48, 72)
    va, vb = _video(40, 60, 90, 4300), _video(30, 120, 180, 4301)          # different lengths and sizes, one scaled size
    boxes_a, boxes_b = _split(box_set(60, 90), [2, 0, 3]), _split(box_set(60, 90)[5:] * 2.0, [1, 4])
    stamps_a, stamps_b = [0.4, 1.0, 1.6], [0.5, 1.1]
    det = KeyframeDetector(dm, DURATION, short_side=48, **KW)
    got = det([va.cuda(), vb.cuda()], [FPS, 15], [stamps_a, stamps_b], [boxes_a, boxes_b])
    want = torch.cat([_oracle_rows(name, g, sd, dtype, va.permute(0, 3, 1, 2).float(), FPS, stamps_a, boxes_a, 48, None, 1),
                      _oracle_rows(name, g, sd, dtype, vb.permute(0, 3, 1, 2).float(), 15, stamps_b, boxes_b, 48, None, 1)])
    _check(got, want, dtype, "two videos f32")
    assert det.chunks == keyframe_chunks([2, 0, 3, 1, 4], 2, 5) and det.forwards == 2
    with pytest.raises(RuntimeError, match="scales to 48 x 64, the deploy form takes 48 x 72"):
        det([va.cuda(), _video(30, 60, 80, 4302).cuda()], FPS, [stamps_a, stamps_b], [boxes_a, boxes_b])


def test_the_clip_at_a_time_form_is_unchanged_after_a_detector_call():
    name, dtype = "resnet_det_r50_small", torch.float32
    dm, sd, g, x, xd, boxes = _form(name, dtype, 48, 72)
    want = _scores(name, g, sd, x, boxes)
    det = KeyframeDetector(dm, DURATION, short_side=48, **KW)
    det(_video(40, 60, 90, 4400).cuda(), FPS, STAMPS[:1], [box_set(60, 90)[:2]])
    got = dm(xd, boxes)                                             # the converted count, after the box buffer held padding rows
    assert (got.cpu() - want).abs().max().item() <= TOL[dtype]
    with pytest.raises(RuntimeError):
        dm(xd, boxes[:2])                                           # still specialised to the box count
    with pytest.raises(RuntimeError):
        dm._pv_load_boxes(torch.zeros(6, 5))
