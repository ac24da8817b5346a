"""Host-only checks of the X3D stem that reads the caller's NCDHW clip (x_src_slot, include/pv_mi355x.h): the plan of
an X3D network has no ingest op and its stem carries a source slot; the library, not Python, decides which stems
qualify (pv_conv3d_ncdhw_supported)."""
import ctypes as C

import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd.accelerator import transmute_model
from pytorchvideo_amd.accelerator.mi355x import tuning
from pytorchvideo_amd.accelerator.mi355x.session import Ptr, Session
from pytorchvideo_amd.models import create_x3d


def _x3d_plan(T, S, B=2):
    m = create_x3d(input_clip_length=T, input_crop_size=S).eval()
    transmute_model(m, "mi355x")
    sess, cur = Session(dtype=torch.bfloat16), None
    for i, b in enumerate(m.blocks):
        b.convert((B, 3, T, S, S) if i == 0 else None, session=sess, input_ref=cur)
        cur = b._out_ref
    return sess, m.blocks[0]._in_ref


@pytest.mark.parametrize("T,S", [(4, 160), (16, 224), (16, 312)])     # X3D-XS / -M / -L geometries
def test_x3d_plan_reads_the_clip_in_the_stem(pv_lib, T, S):
    sess, x_in = _x3d_plan(T, S)
    assert all(kind != L.OP_INGEST for kind, *_ in sess.ops)
    stem = sess.ops[0][2]
    assert sess.ops[0][3].startswith("stem.conv01")
    assert isinstance(stem["x_src_slot"], Ptr) and stem["x_src_slot"].space == "weights"
    assert stem["x_src_c"] == 3 and stem["x"].off == x_in.off       # slot 0: the 4-channel buffer of the ingest
    assert x_in.src_slot is stem["x_src_slot"] and x_in.c4_readers == 0
    assert sum(1 for o in sess.ops if o[2].get("x_src_slot") is not None) == 1


def test_knob_off_gives_the_parent_plan(pv_lib):
    tuning.OPTIONS["stem_ncdhw"] = False
    try:
        sess, x_in = _x3d_plan(4, 160)
    finally:
        tuning.OPTIONS["stem_ncdhw"] = True
    assert "x_src_slot" not in sess.ops[0][2] and x_in.src_slot is None and x_in.c4_readers == 1


def _stem_desc(**kw):
    d = L.Conv3dDesc()
    g = dict(B=2, Ti=16, Hi=224, Wi=224, To=16, Ho=112, Wo=112, cin=4, ldx=4, ldy=24, cout=24, dtype=L.PV_BF16,
             kt=1, kh=3, kw=3, st=1, sh=2, sw=2, pt=0, ph=1, pw=1, dwt_k=5, act=L.ACT_RELU, x_src_c=3,
             x_bs=16 * 224 * 224 * 4, y_bs=16 * 112 * 112 * 24)
    g.update(kw)
    for k, v in g.items():
        setattr(d, k, v)
    return d


def test_library_decides_which_stems_read_the_clip(pv_lib):
    ok = lambda **kw: pv_lib.pv_conv3d_ncdhw_supported(C.byref(_stem_desc(**kw)))
    assert ok() == 1
    assert ok(dwt_k=3) == 1 and ok(x_src_c=1) == 1 and ok(x_src_c=4) == 1
    assert ok(Hi=37, Wi=53, Ho=19, Wo=27) == 1                       # odd sizes: element loads
    assert ok(x_src_c=0) == 0 and ok(x_src_c=5) == 0
    assert ok(kh=5, kw=5, ph=2, pw=2) == 0                            # not X3D's conv_xy
    assert ok(sh=1, sw=1, Ho=224, Wo=224) == 0
    assert ok(dwt_k=0) == 0 and ok(dwt_k=7) == 0                      # the temporal conv is part of the kernel
    assert ok(B=512) == 0                                             # 31-bit element offsets
    assert pv_lib.pv_conv3d_ncdhw_supported(None) == 0
