"""The res5 of a ResNeXt-3D detection backbone through the emitter (no GPU): conv_b dilated (1, 2, 2) at stride 1 with 32
channels per group is planned as a grouped pv_conv3d with compact weights in bf16; fp32, and bf16 with the tuning key off,
keep the block-diagonal dense route."""
import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd.accelerator import transmute_model
from pytorchvideo_amd.accelerator.mi355x import tuning
from pytorchvideo_amd.accelerator.mi355x.session import Session
from pytorchvideo_amd.models import create_resnet


@pytest.mark.parametrize("dtype,key", [(torch.bfloat16, True), (torch.bfloat16, False), (torch.float32, True)],
                         ids=["bf16", "bf16_key_off", "fp32"])
def test_dilated_resnext_res5_routes(dtype, key, monkeypatch):
    monkeypatch.setitem(tuning.OPTIONS, "grouped_conv_dilated", key)
    m = create_resnet(model_depth=50, model_num_class=5, stem_dim_out=128, stage_conv_b_num_groups=(32, 32, 32, 32),
                      stage_conv_b_dilation=((1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 2, 2)), head_pool_kernel_size=(4, 4, 4),
                      stage_spatial_h_stride=(1, 2, 2, 1), stage_spatial_w_stride=(1, 2, 2, 1)).eval()
    transmute_model(m, "mi355x")
    sess, cur = Session(dtype=dtype), None
    for i, b in enumerate(m.blocks):
        b.convert((1, 3, 4, 64, 64) if i == 0 else None, session=sess, input_ref=cur)
        cur = b._out_ref
    res5 = [o for o in sess.ops if o[3].split("|")[0] == "conv_b"][13:]
    assert len(res5) == 3 and all(o[0] == L.OP_CONV3D for o in res5)
    g = 32 if dtype == torch.bfloat16 and key else 0          # 32 groups of 32 channels, or dense
    for f in (o[2] for o in res5):
        assert (f["cout"], f["kh"], f["sh"], f["dil_h"], f["dil_w"], f["ph"], f["Ho"], f["Wo"]) == (1024, 3, 1, 2, 2, 2, 4, 4)
        assert f["groups"] == g and dict(sess._weights)[f["w"].off].numel() == 1024 * 9 * (g or 1024)
