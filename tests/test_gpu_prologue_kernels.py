"""The kernels whose start-up issues every request before its first wait (filter slab, BatchNorm tables, the first group's
operands and gate rows ahead of the barrier), at the smallest shapes where that start-up can go wrong: far fewer voxel groups
than resident workgroups (almost every workgroup is padded and must touch nothing), wave tiles and groups that straddle clip
boundaries, a last clip with no next clip for the gate cache, ragged channel slabs and zero-filled K tails.

Operands sit at the very END of their allocations behind a NaN guard and outputs between canaries: a load the padded
workgroups or the rows past M failed to suppress lands past the allocation or poisons the result, a stray store hits a
canary.  References are fp32 torch on the same bf16-rounded operands with the tolerances of tests/test_gpu_kernels.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
from gpu_util import _routed_kernel, call, rel_err
import test_gpu_kernels as K

pytestmark = pytest.mark.gpu
CANARY = 7.0


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _at_end(values, dtype, guard=4096):
    """`values` as the LAST elements of a device allocation, NaN in front: (view, keep-alive)."""
    buf = torch.full((guard + values.numel(),), float("nan"), dtype=dtype, device="cuda")
    view = buf[guard:].view(values.shape)
    view.copy_(values.to(dtype))
    return view, buf


def _guarded(shape, dtype, guard=4096):
    """An output buffer between two canary regions: (view, whole)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((2 * guard + n,), CANARY, dtype=dtype, device="cuda")
    return buf[guard:guard + n].view(shape), buf


def _guards_intact(whole, n, guard=4096):
    return bool(torch.all(whole[:guard] == CANARY)) and bool(torch.all(whole[guard + n:] == CANARY))


def _pad8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------ pw_stream_kernel, one operand
@pytest.mark.parametrize("B,S,cin,cout,gate,res,f32", [
    (3, 81, 216, 96, True, True, False),     # gated whole-K conv_c of res4: KS 7, 4 groups, 16- and 64-voxel tiles across clips
    (3, 81, 216, 96, False, False, False),   # the same without gate and residual: XFORM false at KS 7
    (1, 100, 96, 96, False, True, True),     # MViT's fp32-output form with an fp32 residual, 100 rows
])
def test_streaming_pointwise_conv_start_up(B, S, cin, cout, gate, res, f32):
    cp = _pad8(cout)
    x, _kx = _at_end(_rand((B, S, cin), 11), torch.bfloat16)
    w, _kw = _at_end(_rand((cout, cin), 12, cin ** -0.5), torch.bfloat16)
    scale, _k1 = _at_end(_rand((cout,), 13) * 0.2 + 1.0, torch.float32)
    shift, _k2 = _at_end(_rand((cout,), 14), torch.float32)
    g, _kg = _at_end(torch.sigmoid(_rand((B, cin), 15)), torch.float32)
    rdt = torch.float32 if f32 else torch.bfloat16
    r, _kr = _at_end(_rand((B, S, cp), 16), rdt)
    xin = x.float()
    if gate:
        xin = xin * g[:, None, :]
        xin = (xin * torch.sigmoid(xin)).bfloat16().float()      # the kernel feeds the MFMA a bf16 operand
    want = F.linear(xin, w.float()) * scale + shift
    if res:
        want = want + r.float()[..., :cout]
    if not f32:
        want = F.relu(want)
    y, whole = _guarded((B, S, cp), rdt)
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.residual = r.data_ptr() if res else None
    d.a_gate = g.data_ptr() if gate else None
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = S * cin, S * cp, S * cp, cin, cp, cp
    Hs, Ws = (9, 9) if S == 81 else (1, S)       # S = 81 is T x H x W = 1 x 9 x 9
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, 1, Hs, Ws, cin, 1, Hs, Ws, cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.a_act, d.dtype = (L.ACT_NONE if f32 else L.ACT_RELU), (L.ACT_SWISH if gate else L.ACT_NONE), L.PV_BF16
    d.y_f32, d.r_f32 = int(f32), int(f32 and res)
    # (ungated layers of more than 128 input channels go to the LDS-DMA GEMM by default: the knob prefers the streaming kernel)
    L.tune(conv_route=1)
    try:
        call("pv_conv3d", d)
        assert _routed_kernel(L.OP_CONV3D, d) == "pw_stream_kernel"
        first = y.clone()
        call("pv_conv3d", d)
    finally:
        L.tune(conv_route=0)
    err = rel_err(first[..., :cout], want)
    print("error %.3e" % err)
    assert err <= 1e-2
    assert torch.all(first[..., cout:] == 0)
    assert _guards_intact(whole, y.numel())
    assert torch.equal(first, y)


# ------------------------------------------------------------------ pw_stream_kernel, projection shortcut as second operand
@pytest.mark.parametrize("cin,cout,cin2,gate", [
    (54, 24, 24, True),      # KS 3: zero-filled K tail (54 is no multiple of 32), ragged rows (24 < 32 output channels)
    (108, 48, 24, False),    # 4 + 1 k-steps: the generic KS 0 form
    (108, 48, 24, True),
])
def test_streaming_pointwise_conv_with_second_operand_start_up(cin, cout, cin2, gate):
    B, T, H, W, st = 2, 2, 5, 7, (1, 2, 2)
    T2, H2, W2 = T, (H - 1) * 2 + 2, (W - 1) * 2 + 1
    cp1, cp2, cpo = _pad8(cin), _pad8(cin2), _pad8(cout)
    hv = torch.zeros(B, T, H, W, cp1)
    hv[..., :cin] = _rand((B, T, H, W, cin), 21)
    h, _kh = _at_end(hv, torch.bfloat16)
    x2v = torch.zeros(B, T2, H2, W2, cp2)
    x2v[..., :cin2] = _rand((B, T2, H2, W2, cin2), 22)
    x2, _k2 = _at_end(x2v, torch.bfloat16)
    w1, w2 = _rand((cout, cin), 23, cin ** -0.5).bfloat16(), _rand((cout, cin2), 24, cin2 ** -0.5).bfloat16()
    shift, _k3 = _at_end(_rand((cout,), 25), torch.float32)
    s1, _k4 = _at_end(_rand((cout,), 26) * 0.2 + 1.0, torch.float32)
    s2, _k5 = _at_end(_rand((cout,), 27) * 0.2 + 0.7, torch.float32)
    g, _kg = _at_end(torch.rand(B, cp1, generator=torch.Generator().manual_seed(28)) * 0.8 + 0.1, torch.float32)
    hp = h[..., :cin].float()
    if gate:
        hp = hp * g[:, :cin].view(B, 1, 1, 1, cin)
        hp = (hp * torch.sigmoid(hp)).bfloat16().float()
    x2s = x2[:, ::st[0], ::st[1], ::st[2], :cin2].float()
    want = F.relu((hp @ w1.float().cuda().t()) * s1 + (x2s @ w2.float().cuda().t()) * s2 + shift)
    k1, k2 = (cin + 31) // 32 * 32, (cin2 + 31) // 32 * 32
    wc = torch.zeros(cout, k1 + k2)
    wc[:, :cin], wc[:, k1:k1 + cin2] = w1.float(), w2.float()
    wcat, _kw = _at_end(wc, torch.bfloat16)
    y, whole = _guarded((B, T, H, W, cpo), torch.bfloat16)
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.shift, d.scale, d.x2_scale = h.data_ptr(), wcat.data_ptr(), y.data_ptr(), shift.data_ptr(), s1.data_ptr(), s2.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cp1, T * H * W * cpo, cp1, cpo
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cp1, T, H, W, cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.dtype = L.ACT_RELU, L.PV_BF16
    if gate:
        d.a_gate, d.a_act = g.data_ptr(), L.ACT_SWISH
    d.x2, d.x2_bs, d.x2_ld, d.x2_cin = x2.data_ptr(), T2 * H2 * W2 * cp2, cp2, cp2
    d.x2_Hi, d.x2_Wi, d.x2_st, d.x2_sh, d.x2_sw = H2, W2, st[0], st[1], st[2]
    assert L.lib().pv_conv3d_x2_supported(C.byref(d)) == 1
    call("pv_conv3d", d)
    assert _routed_kernel(L.OP_CONV3D, d) == "pw_stream_kernel"
    err = rel_err(y[..., :cout], want)
    print("error %.3e" % err)
    assert err <= 1e-2
    assert torch.all(y[..., cout:] == 0)
    assert _guards_intact(whole, y.numel())


# ------------------------------------------------------------------ tap_stream_kernel
@pytest.mark.parametrize("B,T,H,W,cin,cout,k,stride", [
    (2, 2, 8, 8, 48, 96, (1, 1, 1), (1, 2, 2)),     # the res4 projection shortcut: strided pointwise, output 2 x 4 x 4
    (2, 3, 5, 5, 32, 32, (3, 1, 1), (1, 1, 1)),     # a (3, 1, 1) conv: three taps in the table
])
def test_tap_streaming_conv_start_up(B, T, H, W, cin, cout, k, stride):
    pad = tuple(kk // 2 for kk in k)
    taps = k[0] * k[1] * k[2]
    x, _kx = _at_end(_rand((B, T, H, W, cin), 31), torch.bfloat16)
    wv = (_rand((cout, cin) + k, 32, (cin * taps) ** -0.5)).bfloat16()
    scale, _k1 = _at_end(torch.rand(cout, generator=torch.Generator().manual_seed(33)) + 0.5, torch.float32)
    shift, _k2 = _at_end(torch.rand(cout, generator=torch.Generator().manual_seed(34)) - 0.5, torch.float32)
    want = F.conv3d(x.float().cpu().permute(0, 4, 1, 2, 3), wv.float(), stride=stride, padding=pad)
    want = F.relu(want * scale.cpu().view(1, -1, 1, 1, 1) + shift.cpu().view(1, -1, 1, 1, 1))
    To, Ho, Wo = want.shape[2:]
    wp, _kw = _at_end(wv.permute(0, 2, 3, 4, 1).reshape(cout, taps, cin).float(), torch.bfloat16)
    y, whole = _guarded((B, To, Ho, Wo, cout), torch.bfloat16)
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), wp.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin, To * Ho * Wo * cout, cin, cout
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin, To, Ho, Wo, cout
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *stride, *pad)
    d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
    call("pv_conv3d", d)
    assert _routed_kernel(L.OP_CONV3D, d) == "tap_stream_kernel"
    err = rel_err(y.permute(0, 4, 1, 2, 3), want)
    print("error %.3e" % err)
    assert err <= 1e-2
    assert _guards_intact(whole, y.numel())


def test_tap_streaming_conv_with_pointwise_conv_behind_it_start_up():
    """Both slabs and both table pairs in the start-up batch: the smallest conv_b -> conv_c case of tests/test_gpu_kernels.py
    (its own references, tolerances and routing assertion)."""
    K.test_conv_b_and_pointwise_conv_c_in_one_launch(1, 3, 9, 9, 16, 36, 20, (3, 3, 3), (1, 1, 1), False, L.ACT_RELU)


# ------------------------------------------------------------------ conv_igemm_kernel, gated
def test_generic_pointwise_conv_gate_staging():
    """432 -> 192 with gate + Swish + residual + ReLU: too wide for the streaming kernel's LDS.  M = 294: the 128-row tiles span
    two clips, the last one is ragged, and the last clip has no next clip for the staged gate rows."""
    B, S, cin, cout = 3, 98, 432, 192
    x, _kx = _at_end(_rand((B, S, cin), 41), torch.bfloat16)
    w, _kw = _at_end(_rand((cout, cin), 42, cin ** -0.5), torch.bfloat16)
    scale, _k1 = _at_end(_rand((cout,), 43) * 0.2 + 1.0, torch.float32)
    shift, _k2 = _at_end(_rand((cout,), 44), torch.float32)
    g, _kg = _at_end(torch.sigmoid(_rand((B, cin), 45)), torch.float32)
    r, _kr = _at_end(_rand((B, S, cout), 46), torch.bfloat16)
    xin = x.float() * g[:, None, :]
    xin = (xin * torch.sigmoid(xin)).bfloat16().float()
    want = F.relu(F.linear(xin, w.float()) * scale + shift + r.float())
    y, whole = _guarded((B, S, cout), torch.bfloat16)
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.residual, d.a_gate = r.data_ptr(), g.data_ptr()
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = S * cin, S * cout, S * cout, cin, cout, cout
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, 2, 7, 7, cin, 2, 7, 7, cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_SWISH, L.PV_BF16
    call("pv_conv3d", d)
    assert _routed_kernel(L.OP_CONV3D, d) == "conv_igemm_kernel"
    err = rel_err(y, want)
    print("error %.3e" % err)
    assert err <= 1e-2
    assert _guards_intact(whole, y.numel())


# ------------------------------------------------------------------ bottleneck_block_kernel
# T shorter than the 4-deep plane pipeline: what the start-up requested is consumed in the first iterations; H = 3 and W = 15
# give a ragged last row tile and a ragged last column tile
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("chans", [(24, 54, 24), (48, 108, 48), (96, 216, 96)])
def test_fused_bottleneck_block_start_up(chans, T):
    K.test_fused_bottleneck_block(chans, 2, T, 3, 15, L.ACT_RELU)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("chans", [(24, 54), (48, 108), (96, 216)])
def test_fused_bottleneck_conv_ab_start_up(chans, T):
    """Mode 1 (stops behind conv_b), partial sums included."""
    K.test_fused_bottleneck_conv_ab_with_squeeze_sums(chans, 2, T, 3, 15)
