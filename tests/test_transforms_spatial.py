"""Host mirrors of the reference's spatial eval transforms (pytorchvideo/transforms/functional.py:92-131,195-231,302-378,
407-446; transforms/transforms.py:100-121,153-175) against outputs of the real reference (tests/golden/spatial_transforms.pt,
made by make_spatial_golden.py); the claim the device path rests on (bilinear resampling commutes with a per-channel affine
map); and everything of pv_resample_crop / DevicePacker that is decided without a GPU."""
import ctypes as C
import types

import pytest
import torch

import spatial_util as SU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

MAX_SCALE = 1.0 / (255.0 * min(SU.STD))


def test_scaled_size_and_crop_offsets_are_the_reference_rules():
    g = SU.golden()
    for i, (shape, size, crop, idxs) in enumerate(SU.CASES):
        hn, wn = TR.scaled_size(shape[2], shape[3], size)
        assert (hn, wn) == tuple(g["scaled_shape"][i][2:])
        assert min(hn, wn) == size
    # functional.py:311-323: centred with ceil; 0 / 2 move the window along the longer side only
    assert TR.crop_offsets(64, 86, 56, 0) == (4, 0) and TR.crop_offsets(64, 86, 56, 1) == (4, 15)
    assert TR.crop_offsets(64, 86, 56, 2) == (4, 30) and TR.crop_offsets(86, 64, 56, 2) == (30, 4)
    assert TR.crop_offsets(86, 64, 56, 0) == (0, 4) and TR.crop_offsets(64, 64, 57, 1) == (4, 4)
    assert TR.crop_offsets(64, 64, 56, 0) == (4, 0) and TR.crop_offsets(64, 64, 56, 2) == (4, 8)   # square: the x rule


def test_short_side_scale_and_uniform_crop_equal_the_reference():
    g = SU.golden()
    for i, (shape, size, crop, idxs) in enumerate(SU.CASES):
        x = SU.normalised(SU.clip(shape, 300 + i))
        assert torch.allclose(x, TR.Normalize(SU.MEAN, SU.STD)(TR.div_255(SU.clip(shape, 300 + i).float())), rtol=0, atol=1e-6)
        scaled = TR.ShortSideScale(size)(x)
        assert tuple(scaled.shape) == tuple(g["scaled_shape"][i])
        for v in idxs:
            got = TR.UniformCropVideo(crop)({"video": scaled, "aug_index": v})["video"]
            assert torch.equal(got, TR.uniform_crop(scaled, crop, v))
            SU.check(got, g["chain"][i][v], shape[2], shape[3], MAX_SCALE, what="host mirror case %d idx %d" % (i, v))
    with pytest.raises(NotImplementedError):
        TR.short_side_scale(torch.zeros(3, 1, 4, 4), 8, backend="opencv")


def test_box_mirrors_equal_the_reference():
    g = SU.golden()
    for i, ((h, w), n, size, crop, v) in enumerate(SU.BOX_CASES):
        ref = g["boxes"][i]
        img = SU.clip((3, 1, h, w), 400 + i).float()
        b0 = SU.boxes(n, h, w, 500 + i)
        scaled, b1 = TR.short_side_scale_with_boxes(img, b0.clone(), size)
        cropped, b2 = TR.uniform_crop_with_boxes(scaled, crop, v, b1.clone())
        assert tuple(cropped.shape) == ref["cropped_shape"]
        for got, want in ((b1, ref["scaled"]), (b2, ref["cropped"]), (TR.clip_boxes_to_image(b0.clone(), h // 2, w // 2), ref["clip_only"]),
                          (TR.crop_boxes(b0.clone(), 7, 3), ref["crop_only"])):
            want = torch.as_tensor(want).float()
            assert got.shape == want.shape
            assert bool(((got - want).abs() <= 1e-6 * torch.clamp(want.abs(), min=1.0)).all())


def test_interpolating_raw_taps_then_the_affine_map_equals_the_reference_chain():
    """scale(norm(x)) == norm(scale(x)) up to fp32 rounding: the header's formula on raw uint8 values, then ch_scale /
    ch_shift, against uniform_crop(short_side_scale(Normalize(Div255(x)))) of the real reference."""
    g = SU.golden()
    scale, shift = SU.affine()
    worst = 0.0
    for i, (shape, size, crop, idxs) in enumerate(SU.CASES):
        u8 = SU.clip(shape, 300 + i)
        hn, wn = TR.scaled_size(shape[2], shape[3], size)
        for v in idxs:
            y, x = TR.crop_offsets(hn, wn, crop, v)
            got = SU.pinned_resample(u8, hn, wn, y, x, crop, crop, scale, shift)
            worst = max(worst, SU.check(got, g["chain"][i][v], shape[2], shape[3], MAX_SCALE, what="commute case %d idx %d" % (i, v)))
    print("worst deviation of the restated formula from the reference chain: %.3e" % worst)


def _desc(keep):
    """A descriptor that passes every check (never launched: each test breaks one field of it)."""
    src, dst = (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    keep.extend([src, dst])
    d = L.ResampleDesc()
    d.src = C.addressof(src) + (-C.addressof(src)) % 16
    d.dst = C.addressof(dst) + (-C.addressof(dst)) % 16
    d.B, d.C, d.T, d.src_T, d.Hs, d.Ws = 1, 3, 1, 1, 2, 2
    d.src_dtype, d.src_layout = L.PV_U8, L.SRC_NCTHW
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = 2, 2, 1, 1, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    return d


def _status(d):
    return L.lib().pv_resample_crop(C.byref(d), None)


def test_resample_rejects_invalid_descriptors_without_a_gpu(pv_lib):
    keep = []
    assert pv_lib.pv_resample_crop(None, None) == L.PV_ERR_INVALID
    assert _status(L.ResampleDesc()) == L.PV_ERR_INVALID
    for field in ("src", "dst"):
        d = _desc(keep)
        setattr(d, field, None)
        assert _status(d) == L.PV_ERR_INVALID
    d = _desc(keep)
    d.C = 5
    assert _status(d) == L.PV_ERR_INVALID
    for nv in (0, 4, -1):
        d = _desc(keep)
        d.n_views = nv
        assert _status(d) == L.PV_ERR_INVALID
    for field, val in (("y_off", 2), ("x_off", 2), ("y_off", -1), ("x_off", -1)):
        d = _desc(keep)
        getattr(d, field)[0] = val
        assert _status(d) == L.PV_ERR_INVALID, field
    d = _desc(keep)
    d.Ho = 3
    assert _status(d) == L.PV_ERR_INVALID
    d = _desc(keep)            # the window of the SECOND view leaves the frame
    d.n_views = 2
    d.x_off[1] = 2
    assert _status(d) == L.PV_ERR_INVALID
    for dtype, ch in ((L.PV_F32, 3), (L.PV_BF16, 3), (L.PV_U8, 4), (L.PV_U8, 1)):
        d = _desc(keep)
        d.src_layout, d.src_dtype, d.C = L.SRC_NTHWC, dtype, ch
        assert _status(d) == L.PV_ERR_INVALID


def test_resample_reports_unsupported_pairs_without_a_gpu(pv_lib):
    keep = []
    d = _desc(keep)
    d.src_dtype = L.PV_BF16                       # planar sources are uint8 or fp32
    assert _status(d) == L.PV_ERR_UNSUPPORTED
    d = _desc(keep)
    d.dst_dtype = L.PV_U8
    assert _status(d) == L.PV_ERR_UNSUPPORTED
    d = _desc(keep)                               # the 4-channel first-layer layout is bf16 only
    d.dst_layout, d.dst_dtype, d.c_p, d.ld, d.bs = L.DST_NDHWC, L.PV_F32, 4, 4, 4
    assert _status(d) == L.PV_ERR_UNSUPPORTED
    d = _desc(keep)
    d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, 12, 16, 16
    assert _status(d) == L.PV_ERR_UNSUPPORTED
    d = _desc(keep)
    d.dst_layout = 7
    assert _status(d) == L.PV_ERR_UNSUPPORTED


def _fake_deployed(batch, size, detection=False):
    ref = types.SimpleNamespace(B=batch, C=3, T=4, H=size, W=size, src_slot=None, c4_readers=0)
    dep = types.SimpleNamespace(_pv_inputs=ref, _pv_session=types.SimpleNamespace(device="cpu"))
    if detection:
        dep._pv_load_boxes = lambda b: None
    return dep


def test_device_packer_rejects_a_crop_that_is_not_the_model_size():
    with pytest.raises(ValueError):
        TR.DevicePacker(_fake_deployed(2, 32), short_side=40, crop_size=28)
    with pytest.raises(ValueError):
        TR.DevicePacker(_fake_deployed(2, 32), short_side=40)          # one without the other
    with pytest.raises(ValueError):
        TR.DevicePacker(_fake_deployed(2, 32), src_layout="NTHWC")     # the interleaved source needs the resampling path
    with pytest.raises(ValueError):
        TR.DevicePacker(_fake_deployed(2, 32), short_side=40, crop_size=32, spatial_idx=(0, 1, 2, 1))
    with pytest.raises(ValueError):
        TR.DevicePacker(_fake_deployed(2, 32), short_side=40, crop_size=32, spatial_idx=3)


def test_device_packer_rejects_a_batch_that_is_not_clips_times_views():
    clip = torch.zeros(2, 3, 4, 48, 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="clips x views"):
        TR.DevicePacker(_fake_deployed(4, 32), short_side=40, crop_size=32, spatial_idx=(0, 1, 2))(clip)
    with pytest.raises(RuntimeError, match="clips x views"):
        TR.DevicePacker(_fake_deployed(4, 32), short_side=40, crop_size=32)(clip)
    with pytest.raises(RuntimeError, match="does not fit"):          # 24 x 64 scaled to 32 x 85 holds a 32 crop; 16 x 64 -> 20 does not
        TR.DevicePacker(_fake_deployed(2, 32), short_side=20, crop_size=32)(clip)
    with pytest.raises(RuntimeError, match="frames"):
        TR.DevicePacker(_fake_deployed(2, 32), short_side=40, crop_size=32)(clip[:, :, :3])


def test_device_packer_rejects_boxes_with_more_than_one_view():
    with pytest.raises(ValueError, match="one view"):
        TR.DevicePacker(_fake_deployed(3, 32, detection=True), short_side=40, crop_size=32, spatial_idx=(0, 1, 2))
    TR.DevicePacker(_fake_deployed(1, 32, detection=True), short_side=40, crop_size=32, spatial_idx=2)   # one view is fine
