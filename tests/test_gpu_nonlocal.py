"""pv_nonlocal_attention (csrc/pv_nlattn.hip) against float64, its descriptor validation, and the non-local block inside
a launch plan.  Sizes are the smallest at which the kernel's 64-row / 64-key tiles can go wrong (see CASES)."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn

from gpu_util import CANARY, TOL, randn, rel_err, stream
from oracle.weights import _calibrate_running_stats, seeded_input, trained_like_fill
from pytorchvideo_amd import _lib as L

pytestmark = pytest.mark.gpu

B, PAD, GAP = 2, 8, 64
CASES = {                      # (Nq, Nk)
    "one_key_tile": (70, 40),  # all masking on the first tile; one full and one ragged row tile
    "ragged_third": (33, 150),  # three key tiles, the last one ragged
    "two_full": (130, 128),    # exactly two key tiles, nothing to mask
    "spike": (64, 400),        # row 17's maximum jumps in the last tile, row 40's in the first
}


def _operands(ci, case, seed=3701):
    nq, nk = CASES[case]
    q, k, v = (randn((B, n, ci), seed + j, 0.5).bfloat16() for j, n in enumerate((nq, nk, nk)))
    if case == "spike":
        k[0, 393], k[0, 2] = 8 * q[0, 17], 8 * q[0, 40]
    return q, k, v


def _reference(q, k, v, mode, scale):
    s = q.double() @ k.double().transpose(1, 2)
    return (torch.softmax(s * scale, -1) if mode == L.NL_SOFTMAX else s * scale) @ v.double()


def _launch(q, k, v, mode, scale, override=()):
    """theta | phi | g as channel slices of ONE buffer (rows past Nq / Nk and the gap between clips hold 100: a key the
    kernel must not see), o with PAD sentinel channels per row and a sentinel gap.  -> (status, o buffer, o rows)"""
    (_, nq, ci), nk = q.shape, k.shape[1]
    rows, ld, ldo = max(nq, nk), 3 * ci + PAD, ci + PAD
    bs, o_bs = rows * ld + GAP, nq * ldo + GAP
    buf = torch.full((B, bs), 100.0, dtype=torch.bfloat16)
    grid = buf[:, :rows * ld].view(B, rows, ld)
    grid[:, :nq, :ci], grid[:, :nk, ci:2 * ci], grid[:, :nk, 2 * ci:3 * ci] = q, k, v
    buf, o = buf.cuda(), torch.full((B, o_bs), CANARY, dtype=torch.bfloat16).cuda()
    d = L.NonLocalAttentionDesc(q=buf.data_ptr(), k=buf.data_ptr() + 2 * ci, v=buf.data_ptr() + 4 * ci, o=o.data_ptr(),
                                q_bs=bs, k_bs=bs, v_bs=bs, o_bs=o_bs, ldq=ld, ldk=ld, ldv=ld, ldo=ldo, B=B, Ci=ci, Nq=nq, Nk=nk,
                                scale=scale, mode=mode, dtype=L.PV_BF16)
    for name, value in dict(override).items():
        setattr(d, name, value)
    status = L.lib().pv_nonlocal_attention(C.byref(d), stream())
    torch.cuda.synchronize()
    o = o.cpu()
    return status, o, o[:, :nq * ldo].view(B, nq, ldo)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode", [L.NL_SOFTMAX, L.NL_DOT_PRODUCT], ids=["softmax", "dot_product"])
@pytest.mark.parametrize("ci", [256, 512])
def test_kernel_against_float64(ci, mode, case):
    q, k, v = _operands(ci, case)
    scale = ci ** -0.5 if mode == L.NL_SOFTMAX else 1.0 / k.shape[1]
    status, o, rows = _launch(q, k, v, mode, scale)
    assert status == L.PV_OK
    err = rel_err(rows[..., :ci], _reference(q, k, v, mode, scale))
    print("ci %d mode %d %s: rel_err %.3e" % (ci, mode, case, err))
    assert err <= TOL[torch.bfloat16]
    assert (rows[..., ci:] == CANARY).all() and (o[:, -GAP:] == CANARY).all()
    if case == "spike" and mode == L.NL_SOFTMAX:      # all of row 17's weight sits on key 393
        assert rel_err(rows[0, 17, :ci], v[0, 393]) <= 2e-2


@pytest.mark.parametrize("override", [dict(Ci=96), dict(Ci=576), dict(mode=2), dict(scale=0.0), dict(k=None), dict(dtype=L.PV_F32)],
                         ids=["ci96", "ci576", "mode2", "scale0", "null_k", "fp32"])
def test_descriptor_rejected_before_launch(override):
    q, k, v = _operands(256, "one_key_tile")
    status, o, _ = _launch(q, k, v, L.NL_SOFTMAX, 0.0625, override)
    assert status in (L.PV_ERR_UNSUPPORTED, L.PV_ERR_INVALID)
    assert (o == CANARY).all()


def _nl_net(instantiation, pool):
    """Two bottleneck blocks around a non-local block, filled like a trained network so that bf16 STORAGE alone stays under
    the 1e-2 bound (oracle/weights.py, trained_like_fill): the BatchNorm that ends the non-local block counts as block-final
    (the paper initialises its gamma to zero, training leaves it small), and theta is scaled by 8, which gives the scores a
    spread of about 1 (0.96 .. 1.4 here).  With the initial spread of 0.1 .. 0.2 the softmax is flat, the block's output is
    nearly the same at every position, its calibrated BatchNorm variance is ~1e-3 and the norm amplifies every rounding:
    the torch module itself, run in bf16 on the CPU, is then 1.7e-2 .. 2.1e-2 away from fp32 (5e-3 .. 7e-3 with this
    fill); the non-local branch is a quarter of the output's magnitude."""
    from pytorchvideo_amd.layers import create_nonlocal
    from pytorchvideo_amd.models.net import Net
    from pytorchvideo_amd.models.resnet import ResStage, create_bottleneck_block, create_res_block

    def block():
        return create_res_block(dim_in=32, dim_inner=8, dim_out=32, bottleneck=create_bottleneck_block,
                                conv_a_stride=(1, 1, 1), conv_b_stride=(1, 1, 1))
    nl = create_nonlocal(dim_in=32, dim_inner=256, pool_size=pool, instantiation=instantiation)
    nl.norm.block_final_bn = True
    return Net(blocks=nn.ModuleList([ResStage(nn.ModuleList([block(), nl, block()]))]))


def _fill(m, x, seed):
    trained_like_fill(m, x, seed)
    nl = m.blocks[0].res_blocks[1]
    with torch.no_grad():
        nl.conv_theta.weight.mul_(8.0)
        nl.conv_theta.bias.mul_(8.0)
    return _calibrate_running_stats(m, x)


@pytest.mark.parametrize("on", [True, False], ids=["kernel", "switched_off"])
@pytest.mark.parametrize("pool", [(1, 2, 2), (1, 1, 1)], ids=["pool", "nopool"])
@pytest.mark.parametrize("instantiation", ["softmax", "dot_product"])
def test_nonlocal_stage_is_one_plan(instantiation, pool, on, monkeypatch):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.accelerator.mi355x import tuning
    monkeypatch.setitem(tuning.OPTIONS, "nonlocal_block", on)
    x = seeded_input((2, 32, 2, 6, 6), 37)          # Nq = 72, Nk = 18 with the pool
    m = _fill(_nl_net(instantiation, pool), x, 37)
    with torch.no_grad():
        want = copy.deepcopy(m)(x)
    transmute_model(m, "mi355x")
    xd = x.cuda().bfloat16()
    rng = torch.get_rng_state()
    dm = convert_to_deployable_form(m, xd, dtype=torch.bfloat16)
    assert torch.equal(torch.get_rng_state(), rng)      # emitting a plan draws nothing from the caller's generator
    with torch.no_grad():
        got = dm(xd)
    kinds = [op[0] for op in dm._pv_session.ops]
    err = rel_err(got, want)
    print("%s pool %s on %s: rel_err %.3e, %d ops" % (instantiation, pool, on, err, len(kinds)))
    assert err <= 1e-2
    if on:
        assert getattr(dm, "_pv_inputs", None) is not None      # nothing declined: one launch plan
        assert kinds.count(L.OP_NONLOCAL) == 1
    else:                                                        # as before: the block stays a torch module
        assert getattr(dm, "_pv_inputs", None) is None and L.OP_NONLOCAL not in kinds


@pytest.mark.parametrize("form", ["net", "detection"])
def test_fp32_conversion_leaves_the_block_in_torch(form):
    """The kernel is bf16 only and the transmuter cannot know the dtype: an fp32 conversion converts the residual blocks one
    by one around the torch module, for a plain net and behind a detection head."""
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import DetectionBBoxNetwork, create_res_roi_pooling_head
    x = seeded_input((2, 32, 2, 6, 6), 37)
    m = _fill(_nl_net("softmax", (1, 2, 2)), x, 37)
    args = (x,)
    if form == "detection":
        head = create_res_roi_pooling_head(in_features=32, out_features=5, resolution=(3, 3), spatial_scale=1.0,
                                           pool_kernel_size=(2, 1, 1), dropout_rate=0.0)
        m = DetectionBBoxNetwork(m, head).eval()
        args = (x, torch.tensor([[0, 0.5, 0.5, 4.0, 5.0], [1, 1.0, 0.0, 5.5, 3.0], [1, 0.0, 2.0, 3.0, 5.0]]))
    with torch.no_grad():
        want = copy.deepcopy(m)(*args)
    transmute_model(m, "mi355x")
    dev = tuple(t.cuda() for t in args)
    dm = convert_to_deployable_form(m, dev if form == "detection" else dev[0], dtype=torch.float32)
    with torch.no_grad():
        got = dm(*dev)
    kinds = [op[0] for op in dm._pv_session.ops]
    assert getattr(dm, "_pv_inputs", None) is None and L.OP_NONLOCAL not in kinds and len(kinds) > 0
    assert rel_err(got, want) <= TOL[torch.float32]
