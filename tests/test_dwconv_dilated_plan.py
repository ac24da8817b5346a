"""The res5 of an ir-CSN-style detection backbone through the emitter (no GPU): a depthwise or 4-per-group (3,3,3) conv_b dilated
(1, 2, 2) is a pv_dwconv3d with the dilation in the descriptor and compact weights; with tuning "dwconv_dilated" off the
depthwise conv is declined and the grouped one is dense.  The new fields fill padding: size and ABI version are unchanged."""
import ctypes as C

import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd.accelerator import transmute_model
from pytorchvideo_amd.accelerator.mi355x import emit, tuning
from pytorchvideo_amd.accelerator.mi355x.session import Session
from pytorchvideo_amd.models import create_resnet


def _res5(gw, key, monkeypatch):
    """-> (session or None where res5 was declined, res5's first conv_b, its three conv_b ops)"""
    monkeypatch.setitem(tuning.OPTIONS, "dwconv_dilated", key)
    m = create_resnet(model_depth=50, model_num_class=5, stem_dim_out=16, stage_conv_b_kernel_size=((3, 3, 3),) * 4,
                      stage_conv_b_num_groups=tuple(c // gw for c in (16, 32, 64, 128)), head_pool_kernel_size=(4, 4, 4),
                      stage_conv_b_dilation=((1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 2, 2)),
                      stage_spatial_h_stride=(1, 2, 2, 1), stage_spatial_w_stride=(1, 2, 2, 1)).eval()
    conv_b = m.blocks[4].res_blocks[0].branch2.conv_b
    transmute_model(m, "mi355x")
    if type(m.blocks[4]).__name__ == "ResStage":          # declined: the stage stayed a torch module
        return None, conv_b, []
    sess, cur = Session(dtype=torch.bfloat16), None
    for i, b in enumerate(m.blocks):
        b.convert((1, 3, 4, 64, 64) if i == 0 else None, session=sess, input_ref=cur)
        cur = b._out_ref
    res5 = [o for o in sess.ops if o[3].split("|")[0] == "conv_b" and 128 in (o[2].get("C"), o[2].get("cout"))]
    assert len(res5) == 3          # res5's three blocks are the only ones 128 channels wide inside
    return sess, conv_b, res5


@pytest.mark.parametrize("gw", [1, 4], ids=["depthwise", "gw4"])
def test_dilated_res5_conv_b_is_a_depthwise_op_with_compact_weights(gw, monkeypatch):
    sess, _, res5 = _res5(gw, True, monkeypatch)
    for kind, _, f, *_ in res5:
        assert kind == L.OP_DWCONV3D and f["gw"] == (gw if gw > 1 else 0)
        assert [f[k] for k in ("C", "kt", "sh", "dil_t", "dil_h", "dil_w", "pt", "ph", "pw", "Ho", "Wo")] == [128, 3, 1, 1, 2, 2, 1, 2, 2, 4, 4]
        assert dict(sess._weights)[f["w"].off].numel() == 27 * gw * 128
    assert not any("dil_h" in o[2] for o in sess.ops if o[0] == L.OP_DWCONV3D and o[2]["C"] < 128)   # undilated ops are as before


def test_key_off_declines_the_depthwise_conv_and_plans_gw4_dense(monkeypatch):
    sess, conv_b, _ = _res5(1, False, monkeypatch)
    assert sess is None
    with pytest.raises(emit.Unsupported):
        emit.check_conv3d(conv_b)
    sess, _, res5 = _res5(4, False, monkeypatch)
    for kind, _, f, *_ in res5:
        assert kind == L.OP_CONV3D and f["groups"] == 0 and (f["dil_h"], f["dil_w"]) == (2, 2)
        assert dict(sess._weights)[f["w"].off].numel() == 128 * 27 * 128       # block-diagonal: 32 x the model's filter


def test_descriptor_size_and_abi_version_are_unchanged():
    D = L.DwConv3dDesc
    assert (C.sizeof(D), D.dil_t.offset, D.pw_w.offset, D.gw.offset, D.dil_h.offset) == (200, 156, 160, 192, 196)
    assert L.lib().pv_version() == 36
