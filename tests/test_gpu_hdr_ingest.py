"""`pv_hdr_views` on the MI355X: PQ / HLG taps of 16-bit YUV 4:2:0 sources converted to BT.709 SDR inside the resampling launch
(include/pv_mi355x.h, "HDR sources"), and the `hdr=` paths of `device_scale_crop`, `DevicePacker` and the predictors.

The reference is tests/hdr_util.py -- the tap rule and the map in float64, straight from the codes, independent of
`transforms` -- followed by `spatial_util.pinned_resample`.  The bound is the one of the 16-bit tests, `spatial_util.bound`,
with the tap term replaced by `4 * E32 * max_scale`: E32 is computed HERE, per launch, as the largest difference over the
launch's own taps between the same restatement evaluated in `torch.float32` on the CPU (tap rule and map, correctly rounded
log / exp / pow / division) and in float64.  That is the fp32 floor of the formulas themselves and knows nothing of the code
under test; the factor 4 is for the device's one-ulp hardware log2 / exp2 / reciprocal (about 7 per channel) and its fused
sums.  Every check prints E32 and the worst deviation before it asserts.

Geometry: the smallest that reaches every branch -- sources of 36 x 52 and 52 x 36 samples, 4 frames, short side 24, crop 20,
T = 2, 2 clips x 3 views; P010 with an odd pitch and I010 with a pitch of W + 4, both with their base one sample into the
buffer; one 2x downscale (rows staged in pairs) and one upscale (rows staged as one run)."""
import collections
from fractions import Fraction

import pytest
import torch

import hdr_util as HU
import orient_util as OU
import spatial_util as SU
import test_gpu_batch_views as BV
import test_gpu_yuv_ingest as G8
import yuv16_util as Y16
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.inference import StreamPredictor, VideoBatchPredictor, VideoPredictor

pytestmark = pytest.mark.gpu
SENTINEL, MAX_SCALE, FORMS, KW = G8.SENTINEL, G8.MAX_SCALE, G8.FORMS, G8.KW
IDS = ["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS]
LAYOUTS = ("P010", "I010")
MATRIX = {"P010": TR.yuv_matrix("bt2020", False, 10, True), "I010": TR.yuv_matrix("bt2020", False, 10)}
SHIFT = {"P010": 6, "I010": 0}
PAD = {"P010": 3, "I010": 4}                                     # pitch - W in samples: odd where the layout allows it
TONE = {"pq": TR.tone_params("pq"), "hlg": TR.tone_params("hlg")}
CODE = {"pq": L.TRANSFER_PQ, "hlg": L.TRANSFER_HLG}
TABLE = torch.tensor([[2, 3], [1, 0]], dtype=torch.int32)        # T = 2 out of 4 frames
SIZE, CROP, IDXS = 24, 20, (0, 1, 2)

Src = collections.namedtuple("Src", "tensor n hs ws geom planes packed")


# ----------------------------------------------------------------------------- sources
def _natural(n, hs, ws, seed, layout):
    """Limited-range codes of ordinary content: luma over the whole nominal range, chroma near neutral -- mostly in gamut."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(64, 941, (n, hs, ws), generator=g, dtype=torch.int64)
    u, v = [torch.randint(448, 577, (n, hs // 2, ws // 2), generator=g, dtype=torch.int64) for _ in range(2)]
    return tuple(p << SHIFT[layout] for p in (y, u, v))


def _random(n, hs, ws, seed, layout):
    """Uniform random codes 0 .. 1023: far out of gamut, every clamp is taken."""
    return Y16.planes(n, hs, ws, seed, shift=SHIFT[layout])


def _source(planes, layout, pitched=True):
    n, hs, ws = planes[0].shape
    kw = dict(pitch=ws + PAD[layout], base=1, garbage=7) if pitched else {}
    packed = Y16.pack(*planes, layout, **kw)
    frames = packed.frames("cuda")
    g = TR.yuv_geometry(frames, layout)
    assert (g["N"], g["Hs"], g["Ws"]) == (n, hs, ws) and (not pitched or frames.data_ptr() % 4 == 2)
    return Src(frames, n, hs, ws, g, planes, packed)


def _own_surfaces(src, seed):
    """The frames of a source as surfaces of their own: int16 allocations 1 or 3 samples in, allocated out of order."""
    cpu = src.packed.frames(dtype=torch.int16)
    n, rows, w = cpu.shape
    pitch = cpu.stride(1)
    own = [None] * n
    for i in torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist():
        buf = torch.full((rows * pitch + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        off = (1, 3)[i % 2]
        buf[off:off + rows * pitch].copy_(torch.as_strided(cpu, (rows * pitch,), (1,), cpu[i].storage_offset()))
        own[i] = torch.as_strided(buf, (rows, w), (pitch, 1), off)
    return own


# ----------------------------------------------------------------------------- launch
def _launch(layout, srcs, orients, triples, form, dtype, transfer, tone=None, size=SIZE, crop=CROP, idxs=IDXS, tables=None,
            surfaces=None, affine=True, window=None, extra=2):
    """pv_hdr_views over `srcs` (record j under orients[j]) for the items `triples` = (source, clip, view) -- or the `window`
    (item0, n) of them, a pointer offset into both copies of the item sequence --; `surfaces`: per source the list of its
    frames as separate allocations, addressed through a pointer table.  Returns the sentinel-filled destination, `extra` items
    longer than the launch."""
    from gpu_util import call
    tables = [TABLE] * len(srcs) if tables is None else tables
    tone = TONE[transfer] if tone is None else tone
    keep = [MATRIX[layout].float().reshape(12).cuda(), tone.float().cuda()]
    ptrs = ptrs_dev = None
    firsts = [None] * len(srcs)
    if surfaces is not None:
        ptrs = torch.tensor([f.data_ptr() for own in surfaces for f in own], dtype=torch.int64)
        ptrs_dev = ptrs.cuda()
        k = 0
        for j, own in enumerate(surfaces):
            firsts[j] = ptrs_dev.data_ptr() + 8 * k
            k += len(own)
    sources = (L.ViewSource * len(srcs))()
    for rec, src, code, first in zip(sources, srcs, orients, firsts):
        hd, wd = OU.displayed_size(src.hs, src.ws, code)
        hn, wn = TR.scaled_size(hd, wd, size)
        assert crop <= hn and crop <= wn
        rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn = (src.tensor.data_ptr() if first is None else first), src.n, src.hs, src.ws, hn, wn
        rec.sy, rec.sx = BV._f32(hd, hn), BV._f32(wd, wn)
        rec.orient = code
        for i, v in enumerate(idxs):
            rec.y_off[i], rec.x_off[i] = TR.crop_offsets(hn, wn, crop, v)
        for f in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch"):
            setattr(rec, f, src.geom[f])
    t = tables[0].shape[1]
    tab, row0 = BV._concat_tables(tables, t + 1)
    items = BV._items([(s, row0[s] + r, v) for s, r, v in triples])
    item0, n = (0, len(items)) if window is None else window
    keep += [BV._upload(sources), BV._upload(items)] + ([x.cuda() for x in SU.affine()] if affine else [])
    h = L.HdrViewsDesc()
    d = h.frames.batch
    d.sources, d.sources_dev = BV.C.addressof(sources), keep[2].data_ptr()
    d.items, d.items_dev = BV.C.addressof(items) + 16 * item0, keep[3].data_ptr() + 16 * item0
    d.n_sources, d.n_items = len(sources), n
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], t + 1, 3, t
    d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U16, L.SRC_YUV420, srcs[0].geom["c_step"], keep[0].data_ptr()
    d.Ho, d.Wo, d.n_views = crop, crop, len(idxs)
    if affine:
        d.ch_scale, d.ch_shift = keep[4].data_ptr(), keep[5].data_ptr()
    dst, cl = G8._destination(form, dtype, n + extra, t, crop)
    BV._set_destination(d, dst, cl, dtype, t, crop)
    if ptrs is not None:
        h.frames.frame_ptrs, h.frames.frame_ptrs_dev, h.frames.n_frame_ptrs = ptrs.data_ptr(), ptrs_dev.data_ptr(), ptrs.numel()
    h.tone, h.transfer = keep[1].data_ptr(), CODE[transfer]
    call("pv_hdr_views", h)
    return dst


def _every(n_sources, n_views=3, clips=2):
    return [(s, r, v) for s in range(n_sources) for r in range(clips) for v in range(n_views)]


# ----------------------------------------------------------------------------- reference, E32, bound
def _sdr(planes, layout, transfer, tone, dtype=torch.float64):
    return HU.to_sdr(HU.rgb_taps(*planes, MATRIX[layout], dtype), transfer, tone, dtype)


def _e32(planes_list, layout, transfer, tone):
    """The largest |float32 restatement - float64 restatement| over the taps of the given planes, in codes."""
    return max(float((_sdr(p, layout, transfer, tone, torch.float32).double() - _sdr(p, layout, transfer, tone)).abs().max())
               for p in planes_list)


def _reference(planes, layout, transfer, tone, table=TABLE, size=SIZE, crop=CROP, idxs=IDXS, affine=True):
    return G8._resampled(_sdr(planes, layout, transfer, tone).float(), table, size, crop, idxs, affine)


def _check(got, ref, hs, ws, e32, max_scale, bf16, what):
    got, ref = got.float().cpu(), ref.float()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    tol = SU.bound(ref, hs, ws, max_scale, bf16) + 4.0 * e32 * max_scale
    worst = err.max().item()
    print("%s: E32 %.3e codes, worst |d| %.3e = %.2f x E32 x scale, smallest bound %.3e, |ref| max %.3f"
          % (what, e32, worst, worst / max(e32 * max_scale, 1e-30), tol.min().item(), ref.abs().max().item()))
    assert bool((err <= tol).all()), "%s: %d elements over the bound, worst %.3e" % (what, int((err > tol).sum()), worst)


# 1. parity with the float64 restatement -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def content():
    """Per (transfer, layout): the two sources of the parity launch -- 36 x 52 natural codes, 52 x 36 uniform random codes, both
    pitched, the base one sample in -- their references and the E32 of their taps; computed once, shared by the forms."""
    cache = {}

    def case(transfer, layout):
        key = (transfer, layout)
        if key not in cache:
            planes = [_natural(4, 36, 52, 1901, layout), _random(4, 52, 36, 1902, layout)]
            refs = [_reference(p, layout, transfer, TONE[transfer]) for p in planes]
            cache[key] = ([_source(p, layout) for p in planes], refs, _e32(planes, layout, transfer, TONE[transfer]))
        return cache[key]
    return case


@pytest.mark.parametrize("form,dtype", FORMS, ids=IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_hdr_views_against_the_float64_restatement(content, transfer, layout, form, dtype):
    srcs, refs, e32 = content(transfer, layout)
    triples = _every(2)
    dst = _launch(layout, srcs, (0, 0), triples, form, dtype, transfer)
    got = G8._planar_of(dst, form, len(triples))
    for s, (src, ref) in enumerate(zip(srcs, refs)):
        _check(got[6 * s:6 * s + 6], ref, src.hs, src.ws, e32, MAX_SCALE, dtype == torch.bfloat16,
               "%s %s %s %s source %d" % (transfer, layout, form, dtype, s))
    assert not torch.equal(got[:6], got[6:])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_hdr_views_sparse_and_dense_staging(transfer, layout):
    """52 x 72 to a short side of 24 (a 2.17x downscale: every output row stages its own two luma rows and their chroma) and
    16 x 24 to the same (upscaled: the strip's source rows staged as one run), in one launch."""
    planes = [_random(4, 52, 72, 1911, layout), _natural(4, 16, 24, 1912, layout)]
    srcs = [_source(p, layout) for p in planes]
    e32 = _e32(planes, layout, transfer, TONE[transfer])
    triples = _every(2)
    for form, dtype in (("planar", torch.bfloat16), ("cl8", torch.float32)):
        got = G8._planar_of(_launch(layout, srcs, (0, 0), triples, form, dtype, transfer), form, len(triples))
        for s, (src, p) in enumerate(zip(srcs, planes)):
            _check(got[6 * s:6 * s + 6], _reference(p, layout, transfer, TONE[transfer]), src.hs, src.ws, e32, MAX_SCALE,
                   dtype == torch.bfloat16, "%s %s %s %d x %d" % (transfer, layout, form, src.hs, src.ws))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_device_error_over_the_fp32_floor(transfer, layout):
    """A 40 x 40 source at a short side of 40, the whole frame as the window: every interpolation weight is exactly 0 or 1, so
    an output IS its tap and |device - float64| is the map's own error.  Natural and uniform random codes, no affine map,
    fp32 planar.  The ratio to E32 is printed (profiles/r19/hdr_ingest.md records it) and held to the bound's factor."""
    table = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32)
    for name, planes in (("natural", _natural(4, 40, 40, 1921, layout)), ("random", _random(4, 40, 40, 1922, layout))):
        src = _source(planes, layout)
        e32 = _e32([planes], layout, transfer, TONE[transfer])
        dst = _launch(layout, [src], (0,), [(0, 0, 0)], "planar", torch.float32, transfer, size=40, crop=40, idxs=(1,),
                      tables=[table], affine=False)
        want = _sdr(planes, layout, transfer, TONE[transfer]).permute(1, 0, 2, 3)[None]
        err = float((dst[:1].double().cpu() - want).abs().max())
        print("%s %s %s: device %.3e codes, E32 %.3e codes, ratio %.2f" % (transfer, layout, name, err, e32, err / e32))
        _check(dst[:1], want, 40, 40, e32, 1.0, False, "%s %s %s taps" % (transfer, layout, name))


# 2. order of operations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_hdr_views_maps_every_tap_before_the_blend(transfer):
    """Alternating black and peak-white columns, downscaled exactly 2x: every output blends a black and a white tap half and
    half.  The launch equals "map, then blend"; "blend, then map" is off by more than 100x the bound."""
    y = torch.full((2, 40, 56), 64, dtype=torch.int64)
    y[:, :, 1::2] = 940
    u = v = torch.full((2, 20, 28), 512, dtype=torch.int64)
    planes = (y, u, v)
    table = torch.tensor([[0, 1]], dtype=torch.int32)
    src = _source(planes, "I010", pitched=False)
    e32 = _e32([planes], "I010", transfer, TONE[transfer])
    dst = _launch("I010", [src], (0,), [(0, 0, 0)], "planar", torch.float32, transfer, size=20, crop=20, idxs=(1,), tables=[table],
                  affine=False)
    want = _reference(planes, "I010", transfer, TONE[transfer], table, 20, 20, (1,), affine=False)
    _check(dst[:1], want, 40, 56, e32, 1.0, False, "%s columns" % transfer)
    blended = G8._resampled(HU.rgb_taps(*planes, MATRIX["I010"]).float(), table, 20, 20, (1,), affine=False)
    wrong = HU.to_sdr(blended.permute(0, 2, 1, 3, 4), transfer, TONE[transfer]).permute(0, 2, 1, 3, 4).float()
    tol = SU.bound(want, 40, 56, 1.0) + 4.0 * e32
    assert bool(((wrong - want).abs() > 100 * tol).any())
    # not a rounding matter: PQ's mid-grey lies 44 codes from the mean of black and white, HLG's (built to degrade gently) 2.7
    assert float((wrong - want).abs().max()) > (20.0 if transfer == "pq" else 1.0)


# 3. exact ties ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tied():
    cache = {}

    def case(layout):
        if layout not in cache:
            planes = [_random(4, 36, 52, 1931, layout), _natural(4, 52, 36, 1932, layout), _random(4, 40, 44, 1933, layout)]
            cache[layout] = (planes, [_source(p, layout) for p in planes])
        return cache[layout]
    return case


@pytest.mark.parametrize("form,dtype", [("planar", torch.bfloat16), ("c4", torch.bfloat16), ("cl8", torch.float32)],
                         ids=["planar_bf16", "c4_bf16", "cl8_f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_items_windows_and_frame_lists_hold_the_same_bits(tied, transfer, layout, form, dtype):
    """Three sources, the items scrambled across them and one repeated: item i equals the one-item launch on its source alone;
    a window of the sequence equals the slice of the whole launch and leaves the sentinel behind; the same frames as separately
    allocated surfaces behind a pointer table give the bits of the whole videos."""
    _, srcs = tied(layout)
    every = _every(3)
    order = torch.randperm(len(every), generator=torch.Generator().manual_seed(1934)).tolist()
    triples = [every[i] for i in order] + [every[order[0]]]
    assert len({s for s, _, _ in triples[:4]}) > 1
    whole = _launch(layout, srcs, (0, 0, 0), triples, form, dtype, transfer)
    n = len(triples)
    assert torch.all(whole[n:] == SENTINEL) and not any(bool(torch.all(whole[i] == SENTINEL)) for i in range(n))
    for i in (0, 5, 11, n - 1):
        s, r, v = triples[i]
        alone = _launch(layout, [srcs[s]], (0,), [(0, r, v)], form, dtype, transfer)
        assert BV._same_bits(whole[i], alone[0]), (i, s, r, v)
        assert torch.all(alone[1:] == SENTINEL)
    for item0, cnt in ((3, 7), (n - 1, 1)):
        part = _launch(layout, srcs, (0, 0, 0), triples, form, dtype, transfer, window=(item0, cnt))
        assert BV._same_bits(part[:cnt], whole[item0:item0 + cnt]) and torch.all(part[cnt:] == SENTINEL), (item0, cnt)
    surfaces = [_own_surfaces(src, 1935 + j) for j, src in enumerate(srcs)]
    assert all(f.data_ptr() % 4 == 2 for own in surfaces for f in own)
    listed = _launch(layout, srcs, (0, 0, 0), triples, form, dtype, transfer, surfaces=surfaces)
    assert BV._same_bits(listed, whole)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_every_orientation_equals_the_upright_launch_on_the_preoriented_copy(tied, transfer, layout):
    """One launch with a record per code 1..7 on the ONE stored video (and code 0 in front: an upright run, then an oriented
    run) against the upright launch on copies oriented beforehand -- the tile kernels against the strips, bit for bit; as a
    frame list too."""
    planes, srcs = tied(layout)
    stored, stored_planes = srcs[0], planes[0]
    codes = (0, 1, 2, 3, 4, 5, 6, 7)
    turned = [stored] + [_preoriented(stored_planes, layout, c) for c in codes[1:]]
    triples = _every(len(codes))
    for form, dtype in (("c4", torch.bfloat16), ("planar", torch.float32)):
        got = _launch(layout, [stored] * len(codes), codes, triples, form, dtype, transfer)
        want = _launch(layout, turned, [0] * len(codes), triples, form, dtype, transfer)
        for i, (s, r, v) in enumerate(triples):
            assert BV._same_bits(got[i], want[i]), "%s %s %s: code %d clip %d view %d" % (transfer, layout, form, codes[s], r, v)
        assert torch.all(got[len(triples):] == SENTINEL) and not BV._same_bits(got[0], got[6])
    surfaces = [_own_surfaces(stored, 1941)] * len(codes)
    listed = _launch(layout, [stored] * len(codes), codes, triples, "c4", torch.bfloat16, transfer, surfaces=surfaces)
    assert BV._same_bits(listed, _launch(layout, [stored] * len(codes), codes, triples, "c4", torch.bfloat16, transfer))


def _preoriented(planes, layout, code):
    frames = OU.yuv_preoriented(*planes, layout, code).frames("cuda")
    g = TR.yuv_geometry(frames, layout)
    return Src(frames, g["N"], g["Hs"], g["Ws"], g, None, None)


def test_the_oriented_items_meet_the_restatement_too():
    """Code 1 (a portrait phone clip, HLG) against the float64 restatement of the pre-oriented planes."""
    planes = _natural(4, 36, 52, 1951, "P010")
    turned = tuple(OU.turned(p, 1) for p in planes)
    e32 = _e32([planes], "P010", "hlg", TONE["hlg"])
    dst = _launch("P010", [_source(planes, "P010")], (1,), _every(1), "planar", torch.float32, "hlg")
    _check(dst[:6], _reference(turned, "P010", "hlg", TONE["hlg"]), 52, 36, e32, MAX_SCALE, False, "hlg P010 code 1")


# 4. finite output ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_all_zero_and_all_ones_surfaces_give_finite_output(transfer):
    """Codes 0 and 0xFFFF everywhere, under the default table, the clip table and an HLG gamma below 1 (a 200-nit display:
    Ys^(gamma - 1) has a negative exponent): log2(0) paths end in 0, nothing is NaN or infinite, in either kernel body."""
    tones = [TONE[transfer], TR.tone_params(transfer, tone_map="clip"), TR.tone_params(transfer, peak_nits=250.0, white_nits=203.0)]
    for value in (0, 0xFFFF):
        planes = tuple(torch.full(s, value, dtype=torch.int64) for s in ((2, 36, 52), (2, 18, 26), (2, 18, 26)))
        table = torch.tensor([[0, 1], [1, 1]], dtype=torch.int32)
        for layout in LAYOUTS:
            src = _source(planes, layout, pitched=False)
            for tone in tones:
                want = _reference(planes, layout, transfer, tone, table, affine=False)
                assert torch.isfinite(want).all()
                for code in (0, 3):
                    dst = _launch(layout, [src], (code,), _every(1), "planar", torch.float32, transfer, tone, tables=[table], affine=False)
                    assert torch.isfinite(dst).all(), (value, layout, code)
                    # a flat frame of saturated taps: every clamp of the map is taken, so nothing of its error is left
                    assert float((dst[:6].cpu() - want).abs().max()) <= 0.01, (value, layout, code)


# 5. predictors ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x3d6():
    return G8._x3d(6)


YUV = ("bt2020", False)


def _p010_video(n, hs, ws, seed, dtype=torch.uint16, **kw):
    return Y16.pack(*Y16.planes(n, hs, ws, seed, shift=6), "P010", **kw).frames("cuda", dtype)


def _composed(dep, video, table, batch, short_side, crop, views, hdr, **geom):
    """The composed path (tests/test_gpu_yuv16_ingest.py): P010 clips materialised by index_select through an int16 view,
    `device_scale_crop(..., src_layout="P010", hdr=)`, the views fed to the deploy form `batch` items at a time, ensembled.
    (video scores, clip scores, the views)."""
    from pytorchvideo_amd.ensemble import VideoEnsembler
    n_clips, t = table.shape
    n_views = len(views)
    v16 = video.view(torch.int16)
    clips = v16.index_select(0, table.reshape(-1).long().to(video.device)).view(n_clips, t, *video.shape[1:])
    x = TR.device_scale_crop(clips, short_side, crop, views, num_frames=t, dtype=torch.bfloat16, src_layout="P010", yuv=YUV, hdr=hdr,
                             **KW, **geom)
    total = n_clips * n_views
    ve = ce = None
    for i0 in range(0, total, batch):
        k = min(batch, total - i0)
        xb = torch.cat([x[i0:i0 + k], torch.full((batch - k,) + tuple(x.shape[1:]), 2.0, dtype=x.dtype, device=x.device)])
        logits = dep(xb)[:k].clone()
        if ve is None:
            ve, ce = VideoEnsembler(1, logits.shape[1], "sum"), VideoEnsembler(n_clips, logits.shape[1], "sum")
        ve.update(logits, [0] * k)
        ce.update(logits, [(i0 + i) // n_views for i in range(k)])
    return ve.result()[0].clone(), ce.result().clone(), x


def test_device_scale_crop_with_hdr_against_the_mirrors():
    """`device_scale_crop(..., hdr=)` on pitched P010 clips against `hdr_to_sdr(yuv420_to_rgb(...))` -- the library's own
    mirrors composed -- and the pinned resample; hdr=None stays the plain 16-bit path."""
    geom = dict(coded_height=40, height=36)
    planes = _natural(4, 36, 52, 1961, "P010")
    packed = Y16.pack(*planes, "P010", coded_height=40, pitch=55, base=1, garbage=3)
    clips = packed.frames("cuda").unflatten(0, (2, 2))
    cpu = packed.frames().unflatten(0, (2, 2))
    for hdr, transfer in (("pq", "pq"), (("hlg", TR.tone_params("hlg", peak_nits=600.0)), "hlg")):
        tone = TR.tone_params("pq") if hdr == "pq" else hdr[1]
        got = TR.device_scale_crop(clips, SIZE, CROP, IDXS, dtype=torch.float32, src_layout="P010", yuv=YUV, hdr=hdr, **KW, **geom)
        rgb = TR.yuv420_to_rgb(cpu, "P010", MATRIX["P010"].float().double(), **geom)            # [2, 2, 3, 36, 52]
        sdr = TR.hdr_to_sdr(rgb, transfer, tone).float().reshape(4, 3, 36, 52)
        want = G8._resampled(sdr, torch.tensor([[0, 1], [2, 3]], dtype=torch.int32), SIZE, CROP, IDXS)
        _check(got, want, 36, 52, _e32([planes], "P010", transfer, tone), MAX_SCALE, False, "device_scale_crop hdr=%s" % transfer)
    plain = TR.device_scale_crop(clips, SIZE, CROP, IDXS, dtype=torch.float32, src_layout="P010", yuv=YUV, **KW, **geom)
    assert torch.equal(plain, TR.device_scale_crop(clips, SIZE, CROP, IDXS, dtype=torch.float32, src_layout="P010", yuv=YUV, hdr=None,
                                                   **KW, **geom))
    assert float((plain - got).abs().max()) > 0.1


def test_predictors_on_a_pq_video(x3d6):
    """x3d_xs, batch 6 = 2 clips x 3 views, the deploy form of the P010 tests.  A 40-frame 64 x 86 P010 surface (pitched, coded
    height 72, the base one sample in) at 10 fps, 5 clips of 8 frames subsampled to 4: `VideoPredictor(..., hdr="pq")` returns
    exactly the scores of the deployed model on `device_scale_crop(..., hdr="pq")` views; a `FrameList` and
    `VideoBatchPredictor` give the same rows; `hdr=None` is another answer."""
    geom = dict(coded_height=72, height=64)
    video = _p010_video(40, 64, 86, 1971, coded_height=72, pitch=96, base=1, garbage=9)
    sampler = D.ConstantClipsPerVideoSampler(Fraction(8, 10), 5)
    args = dict(short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV)
    pred = VideoPredictor(x3d6, sampler, hdr="pq", **args, **KW, **geom)
    table, _ = D.clip_frame_table(sampler, 40, 10, pred.packer.clip_frames)
    scores, clip_scores = pred(video, 10, return_clip_scores=True)
    scores, clip_scores = scores.clone(), clip_scores.clone()
    want, want_clips, _ = _composed(x3d6, video, table, 6, 176, 160, (0, 1, 2), "pq", **geom)
    assert torch.equal(scores, want), "video scores differ by %.3e" % (scores - want).abs().max().item()
    assert torch.equal(clip_scores, want_clips) and not torch.equal(clip_scores[0], clip_scores[-1])
    frames = TR.FrameList(list(video.unbind(0)), src_layout="P010")
    assert torch.equal(pred(frames, 10), scores)
    # hdr=None is the plain P010 path, and another answer; so is the other transfer
    plain = VideoPredictor(x3d6, sampler, **args, **KW, **geom)(video, 10).clone()
    assert not torch.equal(plain, scores)
    hlg = VideoPredictor(x3d6, sampler, hdr="hlg", **args, **KW, **geom)(video, 10).clone()
    assert not torch.equal(hlg, scores) and not torch.equal(hlg, plain)
    # many videos per forward
    other = _p010_video(17, 70, 60, 1972, dtype=torch.int16)
    want_other = VideoPredictor(x3d6, sampler, hdr="pq", **args, **KW)(other, 10).clone()
    both = VideoBatchPredictor(x3d6, sampler, hdr="pq", **args, **KW)
    got = both([video.view(torch.int16), other], 10, height=[64, None], coded_height=[72, None])
    assert torch.equal(got[0], scores) and torch.equal(got[1], want_other) and not torch.equal(got[0], got[1])
    # a batch of materialised clips through DevicePacker.__call__, and one video through fill_video
    clips = torch.as_strided(video, (2, 4) + tuple(video.shape[1:]), (4 * video.stride(0),) + tuple(video.stride()),
                             video.storage_offset() + 8 * video.stride(0))
    packer = TR.DevicePacker(x3d6, hdr="pq", **args, **KW, **geom)
    logits = packer(clips).clone()
    views = TR.device_scale_crop(clips, 176, 160, (0, 1, 2), src_layout="P010", yuv=YUV, hdr="pq", **KW, **geom)
    assert torch.equal(logits, x3d6(views).clone())
    # a portrait HLG phone clip: the stored frames under "rotate 90" equal the copy turned beforehand
    stored_planes = Y16.planes(12, 64, 86, 1973, shift=6)
    stored = Y16.pack(*stored_planes, "P010").frames("cuda")
    upright = OU.yuv_preoriented(*stored_planes, "P010", 1).frames("cuda")
    phone = VideoPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10)), hdr="hlg", **args, **KW)
    assert torch.equal(phone(stored, 10, orientation=TR.orientation_code(90)).clone(), phone(upright, 10))


def test_stream_predictor_on_pq_surfaces(x3d6):
    """One push of 23 P010 surfaces (each an allocation of its own) scores the 6 windows `VideoPredictor` scores offline."""
    dur, stride, fps = Fraction(8, 10), Fraction(3, 10), 10
    video = _p010_video(23, 64, 86, 1981)
    surfaces = [f.clone() for f in video.view(torch.int16).unbind(0)]
    args = dict(short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV, hdr="pq")
    clip_scores = VideoPredictor(x3d6, D.UniformClipSampler(dur, stride), **args, **KW)(video, fps, return_clip_scores=True)[1].clone()
    assert tuple(clip_scores.shape) == (6, 400)
    sp = StreamPredictor(x3d6, dur, stride, fps, **args, **KW)
    out = sp.push(surfaces)
    assert [k for k, _, _ in out] == list(range(6))
    for k, _, s in out:
        assert torch.equal(s, clip_scores[k]), k
    assert not torch.equal(out[0][2], out[5][2])
    plain = StreamPredictor(x3d6, dur, stride, fps, **{**args, "hdr": None}, **KW).push(surfaces)
    assert not torch.equal(plain[0][2], out[0][2])
