"""pv_resample_crop on the MI355X: short_side_scale + uniform_crop fused into the ingest (include/pv_mi355x.h), through
`transforms.device_scale_crop`, the raw C ABI (every destination form) and `DevicePacker` on converted models.

References: the real reference's outputs (tests/golden/spatial_transforms.pt) at small sizes, the host mirrors (pinned to
those fixtures by tests/test_transforms_spatial.py) on the CPU at full geometry, and for whole models the SAME deploy form
fed the host-transformed views through the existing packer.  Tolerances: spatial_util.bound (derived, not tuned)."""
import os

import pytest
import torch

import spatial_util as SU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

pytestmark = pytest.mark.gpu
MAX_SCALE = 1.0 / (255.0 * min(SU.STD))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _host_views(clip_u8, size, crop, idxs, normalise=True, num_frames=None):
    """[B*n_views, C, T, crop, crop] fp32 on the CPU: the host mirrors, clip by clip and view by view."""
    out = []
    for b in range(clip_u8.shape[0]):
        x = clip_u8[b]
        if num_frames is not None:
            x = TR.uniform_temporal_subsample(x, num_frames)
        x = SU.normalised(x) if normalise else x.float()
        scaled = TR.short_side_scale(x, size)
        out.extend(TR.uniform_crop(scaled, crop, v) for v in idxs)
    return torch.stack(out)


@pytest.mark.parametrize("layout", ["NCTHW", "NTHWC"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_device_scale_crop_equals_the_reference_fixtures(layout, dtype):
    g = SU.golden()
    worst = 0.0
    for i, (shape, size, crop, idxs) in enumerate(SU.CASES):
        u8 = SU.clip(shape, 300 + i)[None]
        src = u8.permute(0, 2, 3, 4, 1).contiguous() if layout == "NTHWC" else u8
        got = TR.device_scale_crop(src.cuda(), size, crop, idxs, SU.MEAN, SU.STD, div255=True, dtype=dtype, src_layout=layout)
        assert got.dtype == dtype and tuple(got.shape) == (len(idxs), 3, shape[1], crop, crop)
        want = torch.stack([g["chain"][i][v] for v in idxs])
        worst = max(worst, SU.check(got, want, shape[2], shape[3], MAX_SCALE, dtype == torch.bfloat16,
                                    "fixture case %d %s %s" % (i, layout, dtype)))
    print("worst deviation from the reference fixtures (%s, %s): %.3e" % (layout, dtype, worst))


@pytest.mark.parametrize("hs,ws,size,crop", [(256, 340, 256, 224), (720, 1280, 256, 224), (480, 270, 356, 312), (128, 171, 256, 224)],
                         ids=["256x340_224", "720p_224", "portrait_312", "upscale_128x171"])
def test_full_geometry_equals_the_host_mirrors(hs, ws, size, crop):
    """Three views, both source layouts, uint8 and fp32 planar sources, bf16 and fp32 results, with frame selection."""
    u8 = SU.clip((2, 3, 3, hs, ws), 600 + hs)
    views = (0, 1, 2)
    want = _host_views(u8, size, crop, views)
    worst = 0.0
    for layout, src in (("NCTHW", u8), ("NTHWC", u8.permute(0, 2, 3, 4, 1).contiguous())):
        for dtype in (torch.float32, torch.bfloat16):
            got = TR.device_scale_crop(src.cuda(), size, crop, views, SU.MEAN, SU.STD, div255=True, dtype=dtype, src_layout=layout)
            worst = max(worst, SU.check(got, want, hs, ws, MAX_SCALE, dtype == torch.bfloat16, "%dx%d %s %s" % (hs, ws, layout, dtype)))
    # fp32 planar source, no affine map, two of three frames: the transform alone
    want_raw = _host_views(u8, size, crop, (2, 0), normalise=False, num_frames=2)
    got = TR.device_scale_crop(u8.float().cuda(), size, crop, (2, 0), num_frames=2, dtype=torch.float32)
    worst = max(worst, SU.check(got, want_raw, hs, ws, 1.0, False, "%dx%d fp32 source, raw" % (hs, ws)))
    # a normalised fp32 source (the order of the reference pipeline itself)
    got = TR.device_scale_crop(SU.normalised(u8[0])[None].cuda(), size, crop, 1, dtype=torch.float32)
    SU.check(got, want[1:2], hs, ws, MAX_SCALE, False, "%dx%d fp32 source, normalised" % (hs, ws))
    print("worst deviation from the host mirrors at %dx%d: %.3e" % (hs, ws, worst))


def _raw(clip, size, crop, idxs, form, dtype, t_index=None, affine=True, layout="NCTHW", item0=0, n_items=0, extra=1):
    """One pv_resample_crop call through the C ABI into a sentinel-filled destination of `extra` more items than written.
    Returns (destination tensor, descriptor)."""
    from gpu_util import call
    d = TR._resample_desc(clip, layout, size, crop, idxs)
    keep = [clip]
    if t_index is not None:
        idx = torch.tensor(t_index, dtype=torch.int32).cuda()
        keep.append(idx)
        d.T, d.t_index = len(t_index), idx.data_ptr()
    if affine:
        scale, shift = [t.cuda() for t in SU.affine()]
        keep.extend([scale, shift])
        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    d.item0, d.n_items = item0, n_items
    n = n_items if n_items else d.B * d.n_views
    d.dst_dtype = L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32
    if form == "planar":
        dst = torch.full((n + extra, d.C, d.T, crop, crop), 7.0, dtype=dtype, device="cuda")
        d.dst_layout = L.DST_NCTHW
    else:
        c_p, ld = {"c4": (4, 4), "cl8": (8, 8), "cl8_ld16": (8, 16), "cl16": (16, 16)}[form]
        dst = torch.full((n + extra, d.T, crop, crop, ld), 7.0, dtype=dtype, device="cuda")
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, c_p, ld, d.T * crop * crop * ld
    d.dst = dst.data_ptr()
    call("pv_resample_crop", d)
    return dst, d


FORMS = [("c4", torch.bfloat16), ("cl8", torch.bfloat16), ("cl8", torch.float32), ("cl8_ld16", torch.bfloat16), ("cl16", torch.float32),
         ("planar", torch.bfloat16), ("planar", torch.float32)]


@pytest.mark.parametrize("form,dtype", FORMS, ids=["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS])
@pytest.mark.parametrize("geom", ["even", "odd_unaligned"])
def test_every_destination_form(form, dtype, geom):
    """Three views of two clips with frame selection and the affine map into each layout the first convolution reads;
    pad channels are zero and nothing behind the last view is touched.  `odd_unaligned`: an odd crop width (no 16-byte
    store lines up) from a source that starts at an odd byte address with an odd row length."""
    if geom == "even":
        shape, size, crop = (2, 3, 5, 97, 131), 64, 56
        u8 = SU.clip(shape, 700)
        dev = u8.cuda()
    else:
        shape, size, crop = (2, 3, 5, 30, 23), 41, 37
        u8 = SU.clip(shape, 701)
        store = torch.zeros(u8.numel() + 1, dtype=torch.uint8, device="cuda")
        store[1:] = u8.reshape(-1).cuda()
        dev = store[1:].view(shape)
        assert dev.data_ptr() % 2 == 1
    views, frames = (0, 1, 2), [4, 0, 3]
    want = _host_views(u8[:, :, frames], size, crop, views)
    dst, d = _raw(dev, size, crop, views, form, dtype, t_index=frames)
    n = 6
    if form == "planar":
        got = dst[:n]
    else:
        got = dst[:n, ..., :3].permute(0, 4, 1, 2, 3)
        assert torch.all(dst[:n, ..., 3:d.c_p] == 0), "pad channels must be zero"
        assert torch.all(dst[:n, ..., d.c_p:] == 7.0), "the voxel stride beyond c_p is not the kernel's to write"
    assert torch.all(dst[n:] == 7.0), "bytes behind the last view were written"
    SU.check(got, want, shape[3], shape[4], MAX_SCALE, dtype == torch.bfloat16, "%s %s %s" % (form, dtype, geom))


def test_channels_last_result_read_back_through_egress():
    """The channels-last form as the library's own egress sees it, without the affine map, from an fp32 source."""
    from gpu_util import call
    shape, size, crop = (1, 3, 2, 49, 67), 32, 28
    u8 = SU.clip(shape, 702)
    dst, _ = _raw(u8.float().cuda(), size, crop, (2,), "cl8", torch.float32, affine=False, extra=0)
    back = torch.empty((1, 3, 2, crop, crop), dtype=torch.float32, device="cuda")
    e = L.LayoutDesc()
    e.src, e.dst = dst.data_ptr(), back.data_ptr()
    e.B, e.C, e.T, e.H, e.W, e.c_p, e.ld, e.bs = 1, 3, 2, crop, crop, 8, 8, 2 * crop * crop * 8
    e.src_dtype, e.dst_dtype = L.PV_F32, L.PV_F32
    call("pv_egress_ncdhw", e)
    SU.check(back, _host_views(u8, size, crop, (2,), normalise=False), 49, 67, 1.0, False, "egress of the cl8 form")


def test_a_launch_writes_only_its_item_range():
    """Items [item0, item0 + n) of the clips x views sequence land at positions 0..n-1 (split-batch deploy forms)."""
    shape, size, crop = (2, 3, 2, 49, 67), 32, 28
    u8 = SU.clip(shape, 703)
    want = _host_views(u8, size, crop, (0, 1, 2))
    for item0, n in ((0, 6), (2, 3), (5, 1)):
        dst, _ = _raw(u8.cuda(), size, crop, (0, 1, 2), "planar", torch.float32, item0=item0, n_items=n)
        SU.check(dst[:n], want[item0:item0 + n], 49, 67, MAX_SCALE, False, "items %d..%d" % (item0, item0 + n))
        assert torch.all(dst[n:] == 7.0)


# ----------------------------------------------------------------------------- DevicePacker on converted models
def _deploy(m, x, dtype=torch.bfloat16, **kw):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    transmute_model(m, "mi355x")
    xd = [t.cuda().to(dtype) for t in x] if isinstance(x, list) else x.cuda().to(dtype)
    return convert_to_deployable_form(m, xd, dtype=dtype, **kw)


def _x3d_xs():
    from oracle.weights import seeded_input, trained_like_fill
    from pytorchvideo_amd.models import create_x3d
    m = create_x3d(model_num_class=400, input_clip_length=4, input_crop_size=160)
    return trained_like_fill(m, seeded_input((4, 3, 4, 160, 160), 5), 0).eval()


def test_packer_resamples_for_x3d_one_view_three_views_and_split_batch():
    """x3d_xs (4 x 160 x 160): logits of the resampling packer against the SAME deploy form fed the host-transformed views
    through the existing packer; bf16 (the stem reads the packer's own NCDHW clip), fp32 (the arena's channels-last
    buffer), three crops folded by VideoEnsembler, and a split-batch form whose boundary cuts a clip's views."""
    from gpu_util import rel_err
    from pytorchvideo_amd.ensemble import VideoEnsembler
    clip = SU.clip((2, 3, 4, 180, 240), 800)
    size, crop = 176, 160
    kw = dict(mean=SU.MEAN, std=SU.STD, div255=True, short_side=size, crop_size=crop)
    host = {v: _host_views(clip, size, crop, (v,)) for v in (0, 1, 2)}
    host3 = _host_views(clip, size, crop, (0, 1, 2))

    dep2 = _deploy(_x3d_xs(), host[1])
    assert dep2._pv_inputs.src_slot is not None and dep2._pv_inputs.c4_readers == 0    # the stem reads an NCDHW clip itself
    single = {}
    for v, layout in ((0, "NCTHW"), (1, "NTHWC"), (2, "NCTHW")):
        want = TR.DevicePacker(dep2)(host[v].cuda()).clone()
        src = clip.permute(0, 2, 3, 4, 1).contiguous() if layout == "NTHWC" else clip
        packer = TR.DevicePacker(dep2, spatial_idx=v, src_layout=layout, **kw)
        single[v] = packer(src.cuda()).clone()
        assert len(packer._planar) == 1                       # resampled into the packer's own bf16 NCDHW clip
        assert rel_err(single[v], want) <= 1e-2, "view %d" % v
    assert rel_err(single[0], single[2]) > 1e-3               # the views are different crops

    dep6 = _deploy(_x3d_xs(), host3)
    want6 = TR.DevicePacker(dep6)(host3.cuda()).clone()
    got6 = TR.DevicePacker(dep6, spatial_idx=(0, 1, 2), **kw)(clip.cuda()).clone()
    assert rel_err(got6, want6) <= 1e-2
    for b in range(2):
        for v in range(3):                                    # item b * 3 + v is view v of clip b: the one-view runs
            assert rel_err(got6[b * 3 + v], single[v][b]) <= 1e-2
    e3 = VideoEnsembler(2, 400)
    e3.update(got6, [0, 0, 0, 1, 1, 1])
    e1 = VideoEnsembler(2, 400)
    for v in range(3):
        e1.update(single[v], [0, 1])
    assert (e3.merge().result() - e1.merge().result()).abs().max().item() <= 1e-2 * e1.result().abs().max().item()

    dep6s = _deploy(_x3d_xs(), host3, streams=3)              # sub-batches of 2 + 2 + 2 items: the cuts fall inside a clip's views
    assert list(dep6s._splits) == [2, 2, 2]
    assert rel_err(TR.DevicePacker(dep6s, spatial_idx=(0, 1, 2), **kw)(clip.cuda()), want6) <= 1e-2

    dep32 = _deploy(_x3d_xs(), host[1], dtype=torch.float32)  # fp32 session: the arena buffer in its own layout
    want32 = TR.DevicePacker(dep32)(host[1].cuda()).clone()
    p32 = TR.DevicePacker(dep32, spatial_idx=1, **kw)
    assert rel_err(p32(clip.cuda()), want32) <= 1e-3 and not p32._planar


def test_packer_resamples_both_slowfast_pathways_from_the_fast_clip():
    """slowfast_r50_small (4 + 16 frames at 96 x 96): the slow pathway is resampled straight from the fast clip through
    t_index; two views of one clip."""
    from gpu_util import rel_err
    from oracle.weights import deterministic_fill
    from pytorchvideo_amd.models import create_slowfast
    g = torch.load(os.path.join(GOLD, "slowfast_r50_small.pt"), weights_only=False)
    m = deterministic_fill(create_slowfast(**g["cfg"]), g["seed"]).eval()
    clip = SU.clip((1, 3, 16, 131, 113), 801)                 # portrait, odd sizes
    size, crop, views = 100, 96, (0, 2)
    fast = _host_views(clip, size, crop, views)
    slow = TR.uniform_temporal_subsample(fast, 4, 2)
    dep = _deploy(m, [slow, fast])
    want = TR.DevicePacker(dep, frame_ratios=(4, 1))(fast.cuda()).clone()
    got = TR.DevicePacker(dep, SU.MEAN, SU.STD, div255=True, frame_ratios=(4, 1), short_side=size, crop_size=crop,
                          spatial_idx=views)(clip.cuda())
    assert tuple(got.shape) == tuple(want.shape) == (2, 32)
    assert rel_err(got, want) <= 1e-2
    with pytest.raises(RuntimeError):
        TR.DevicePacker(dep, frame_ratios=(4, 1), short_side=size, crop_size=crop)(clip.cuda())   # 1 clip x 1 view != 2


def test_packer_resamples_for_a_detection_model_and_moves_the_boxes():
    """resnet_det_r50_small (4 x 64 x 64, 6 boxes): boxes given in source pixels follow the clip through the box mirrors."""
    from oracle.weights import detection_fill
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet_with_roi_head
    g = torch.load(os.path.join(GOLD, "resnet_det_r50_small.pt"), weights_only=False)
    m = detection_fill(create_resnet_with_roi_head(**g["cfg"]), g["seed"]).eval()
    clip = SU.clip((2, 3, 4, 90, 120), 802)
    size, crop, v = 72, 64, 2
    boxes = g["boxes"].clone()
    boxes[:, 1:] *= 1.5                                       # spread over the 90 x 120 source frame
    host = _host_views(clip, size, crop, (v,))
    _, scaled_boxes = TR.short_side_scale_with_boxes(clip[0].float(), boxes[:, 1:].clone(), size)
    _, host_boxes = TR.uniform_crop_with_boxes(torch.zeros(3, 1, 72, 96), crop, v, scaled_boxes)
    host_boxes = torch.cat([boxes[:, :1], host_boxes], 1)
    transmute_model(m, "mi355x")
    dm = convert_to_deployable_form(m, (host.cuda().bfloat16(), host_boxes), dtype=torch.bfloat16)
    want = TR.DevicePacker(dm)(host.cuda(), host_boxes).clone()
    got = TR.DevicePacker(dm, SU.MEAN, SU.STD, div255=True, short_side=size, crop_size=crop, spatial_idx=v)(clip.cuda(), boxes).clone()
    assert tuple(got.shape) == tuple(want.shape)
    assert (got - want).abs().max().item() <= 2.5e-2          # the detection tests' bf16 bound on sigmoid scores
    moved = boxes.clone()
    moved[:, 1:] = moved[:, 1:] * 0.5 + 3.0
    got2 = TR.DevicePacker(dm, SU.MEAN, SU.STD, div255=True, short_side=size, crop_size=crop, spatial_idx=v)(clip.cuda(), moved)
    assert (got2 - got).abs().max().item() > 2.5e-2           # the boxes are data
