"""The X3D stem that reads the caller's NCDHW clip itself (x_src_slot, include/pv_mi355x.h; csrc/pv_stem.hip
stem_dir_dwt_kernel): bit-identical to the ingest + 4-channel stem it replaces, on every load path of the kernel
(16-byte planes, element loads for odd widths / misaligned clips, the 4-channel buffer after a fallback ingest),
and a captured graph that follows the input's address."""
import pytest
import torch
import torch.nn as nn

from oracle.weights import seeded_input

pytestmark = pytest.mark.gpu


def _stem_net(kt, seed):
    from pytorchvideo_amd.models.net import Net
    from pytorchvideo_amd.models.x3d import create_x3d_stem
    torch.manual_seed(seed)
    stem = create_x3d_stem(in_channels=3, out_channels=24, conv_kernel_size=(kt, 3, 3), conv_padding=(kt // 2, 1, 1))
    m = Net(blocks=nn.ModuleList([stem]))
    bn = stem.norm
    with torch.no_grad():
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
    return m.eval()


def _deploy(kt, x, direct, seed=0, streams=1, use_graph=True):
    """The stem alone as a whole-net plan; direct=False is the ingest + 4-channel stem of the parent commit."""
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.accelerator.mi355x import tuning
    m = _stem_net(kt, seed)
    transmute_model(m, "mi355x")
    old = tuning.OPTIONS["stem_ncdhw"]
    tuning.OPTIONS["stem_ncdhw"] = direct
    try:
        dm = convert_to_deployable_form(m, x, dtype=torch.bfloat16, streams=streams, use_graph=use_graph)
    finally:
        tuning.OPTIONS["stem_ncdhw"] = old
    for s in getattr(dm, "_pv_sessions", [dm._pv_session]):
        assert (s.ops[0][2].get("x_src_slot") is not None) == direct
    return dm


def _run(dm, x):
    out = dm(x)
    return out.clone() if not isinstance(out, list) else [o.clone() for o in out]


def _slots(dm):
    return [v for s in getattr(dm, "_pv_sessions", [dm._pv_session]) for v in s._slot_vals.values()]


def _clip(shape, seed):
    return seeded_input(shape, seed).cuda().bfloat16()


@pytest.mark.parametrize("shape,kt", [
    ((2, 3, 16, 64, 64), 5),      # 16-byte plane loads, B > 1
    ((1, 3, 7, 33, 40), 5),       # partial tiles, T not a multiple of the ring
    ((3, 3, 2, 37, 53), 5),       # odd H / W: element loads; T shorter than the ring
    ((1, 3, 5, 48, 48), 3),       # 3-tap temporal conv
])
def test_fused_stem_is_bit_identical_to_ingest_plus_stem(shape, kt):
    x = _clip(shape, 1)
    ref, new = _deploy(kt, x, False), _deploy(kt, x, True)
    want = _run(ref, x)
    got = _run(new, x)
    assert _slots(new) == [x.data_ptr()]           # the stem read the caller's clip: no ingest
    assert torch.equal(got, want)


def test_misaligned_clip_is_bit_identical():
    shape = (2, 3, 6, 40, 48)
    n = 1
    for v in shape:
        n *= v
    buf = _clip((n + 8,), 2).reshape(-1)
    x = buf[1:1 + n].view(shape)                     # 2-byte aligned base address
    assert x.data_ptr() % 16 == 2 and x.is_contiguous()
    ref, new = _deploy(5, x, False), _deploy(5, x, True)
    want = _run(ref, x.clone())
    assert torch.equal(_run(new, x), want)
    assert _slots(new) == [x.data_ptr()]


def test_two_inputs_two_results_single_plan_and_joint_graph():
    shape = (4, 3, 8, 64, 64)
    x1, x2 = _clip(shape, 3), _clip(shape, 4)
    ref = _deploy(5, x1, False)
    w1, w2 = _run(ref, x1), _run(ref, x2)
    assert not torch.equal(w1, w2)
    for streams in (1, 2):
        new = _deploy(5, x1, True, streams=streams)
        assert torch.equal(_run(new, x1), w1)
        assert torch.equal(_run(new, x2), w2)      # the replay followed the new address
        assert torch.equal(_run(new, x1), w1)
    x2.copy_(x1)                                   # same address, new content: read at replay time
    assert torch.equal(_run(new, x2), w1)


def test_fallback_forms_route_through_the_ingest_and_match():
    from pytorchvideo_amd.transforms import DevicePacker
    shape = (2, 3, 8, 48, 48)
    x = _clip(shape, 5)
    ref, new = _deploy(5, x, False), _deploy(5, x, True)
    want = _run(ref, x)
    assert torch.equal(_run(new, x), want) and _slots(new) == [x.data_ptr()]
    # non-contiguous clip (same values): ingest, slot back to the 4-channel buffer
    xs = x.transpose(3, 4).contiguous().transpose(3, 4)
    assert not xs.is_contiguous()
    assert torch.equal(_run(new, xs), want) and _slots(new) == [0]
    # fp32 clip
    assert torch.equal(_run(new, x.float()), _run(ref, x.float())) and _slots(new) == [0]
    # back to the direct form
    assert torch.equal(_run(new, x), want) and _slots(new) == [x.data_ptr()]
    # uint8 + Div255 / Normalize (DevicePacker's channel affine) and frame selection (t_index)
    u8 = (seeded_input((2, 3, 16, 48, 48), 6).abs() * 60).clamp(0, 255).to(torch.uint8).cuda()
    for clip, ratio in ((u8[:, :, :8].contiguous(), 1), (u8, 2)):   # 8 frames: affine only; 16 frames: t_index too
        norm = dict(mean=[0.45, 0.45, 0.45], std=[0.225, 0.225, 0.225], div255=True, frame_ratios=(ratio,))
        pk_ref, pk_new = DevicePacker(ref, **norm), DevicePacker(new, **norm)
        want_u8 = pk_ref(clip).clone()
        assert torch.equal(pk_new(clip).clone(), want_u8) and _slots(new) == [0]
    pk = DevicePacker(new, frame_ratios=(2,))                        # bf16 with frame selection only
    x16 = _clip((2, 3, 16, 48, 48), 8)
    assert torch.equal(pk(x16).clone(), _run(ref, x16[:, :, pk._t_index(16, pk.refs[0]).long()])) and _slots(new) == [0]
    # a bf16 clip through DevicePacker with nothing to apply is served in place
    pk = DevicePacker(new)
    assert torch.equal(pk(x).clone(), want) and _slots(new) == [x.data_ptr()]


def test_x3d_s_logits_unchanged():
    """A whole X3D network (stem + residual stages + head): the same logits, bit for bit, through the joint graph."""
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.accelerator.mi355x import tuning
    from pytorchvideo_amd.models import create_x3d
    from oracle.weights import trained_like_fill
    T, S = 13, 160
    x = _clip((4, 3, T, S, S), 7)
    outs = []
    for direct in (False, True):
        m = create_x3d(model_num_class=400, input_clip_length=T, input_crop_size=S)
        trained_like_fill(m, seeded_input((4, 3, T, S, S), 5), 0)
        transmute_model(m, "mi355x")
        tuning.OPTIONS["stem_ncdhw"] = direct
        try:
            dm = convert_to_deployable_form(m, x, dtype=torch.bfloat16, streams=2)
        finally:
            tuning.OPTIONS["stem_ncdhw"] = True
        outs.append(dm(x).float().cpu())
        assert _slots(dm) == ([x[:2].data_ptr(), x[2:].data_ptr()] if direct else [])
    assert torch.equal(outs[0], outs[1])
