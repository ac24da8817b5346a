"""ResNeXt-3D stage layout through the emitter (no GPU): conv_b with 16 / 32 channels per group is planned as a grouped
pv_conv3d (pv_conv3d_desc.groups, compact weights), 4 / 8 per group stay in the depthwise kernel, fp32 keeps the
block-diagonal dense route."""
import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd.accelerator import transmute_model
from pytorchvideo_amd.accelerator.mi355x.session import Session
from pytorchvideo_amd.models import create_resnet


def _plan(dtype):
    m = create_resnet(model_depth=50, model_num_class=5, stem_dim_out=128, stage_conv_b_num_groups=(32, 32, 32, 32),
                      head_pool_kernel_size=(4, 2, 2)).eval()
    transmute_model(m, "mi355x")
    sess, cur = Session(dtype=dtype), None
    for i, b in enumerate(m.blocks):
        b.convert((1, 3, 4, 64, 64) if i == 0 else None, session=sess, input_ref=cur)
        cur = b._out_ref
    convs_b = [o for o in sess.ops if o[3].split("|")[0] == "conv_b"]
    assert len(convs_b) == 16                                      # 3 + 4 + 6 + 3 bottlenecks
    return sess, convs_b


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_resnext_conv_b_routes(dtype):
    sess, convs_b = _plan(dtype)
    numel = lambda o: dict(sess._weights)[o[2]["w"].off].numel()
    res23, res45 = convs_b[:7], convs_b[7:]
    assert [o[2]["gw"] for o in res23] == [4] * 3 + [8] * 4 and all(o[0] == L.OP_DWCONV3D for o in res23)
    assert all(o[0] == L.OP_CONV3D for o in res45)
    for o, (c, gw) in zip(res45, [(512, 16)] * 6 + [(1024, 32)] * 3):
        f = o[2]
        assert f["cout"] == c and f["kt"] * f["kh"] * f["kw"] == 9
        if dtype == torch.bfloat16:
            assert f["groups"] == 32 and numel(o) == c * 9 * gw
        else:
            assert f["groups"] == 0 and numel(o) == c * 9 * c
