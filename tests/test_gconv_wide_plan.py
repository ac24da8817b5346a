"""ResNeXt-3D 32x8d stage layout through the emitter (no GPU): inner widths 256 / 512 / 1024 / 2048 over 32 groups are 8 / 16 /
32 / 64 channels per group; res5's conv_b (64 per group) is planned as a grouped pv_conv3d with compact weights
(csrc/pv_gconv_wide.hip), not as a block-diagonal dense conv."""
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd.accelerator import transmute_model
from pytorchvideo_amd.accelerator.mi355x.session import Session
from pytorchvideo_amd.models import create_resnet


def test_resnext_32x8d_res5_conv_b_is_grouped():
    m = create_resnet(model_depth=50, model_num_class=5, stem_dim_out=256, stage_conv_b_num_groups=(32, 32, 32, 32),
                      head_pool_kernel_size=(4, 2, 2)).eval()
    transmute_model(m, "mi355x")
    sess, cur = Session(dtype=torch.bfloat16), None
    for i, b in enumerate(m.blocks):
        b.convert((1, 3, 4, 64, 64) if i == 0 else None, session=sess, input_ref=cur)
        cur = b._out_ref
    convs_b = [o for o in sess.ops if o[3].split("|")[0] == "conv_b"]
    assert len(convs_b) == 16                                      # 3 + 4 + 6 + 3 bottlenecks
    weights = dict(sess._weights)
    for o, (c, gw) in zip(convs_b[3:], [(512, 16)] * 4 + [(1024, 32)] * 6 + [(2048, 64)] * 3):
        f = o[2]
        assert o[0] == L.OP_CONV3D and f["cout"] == c and f["kt"] * f["kh"] * f["kw"] == 9
        assert f["groups"] == 32 and weights[f["w"].off].numel() == c * 9 * gw
