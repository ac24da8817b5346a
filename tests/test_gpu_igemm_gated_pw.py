"""conv_igemm_kernel on pointwise bf16 layers: the buffer-addressed operand path (every K step issues the same loads, rows past M,
channels past cout and the K tail come back as zero from the range check) at the smallest shapes that reach each of its edges.

  K steps   cin 32 (one step), 40 (two, ragged tail), 72 (three: the loop body runs once and one step is left behind it),
            432 (14 steps, half-empty last one: X3D res5's conv_c)
  channels  192 and 200 output channels (two 128-channel tiles, the second one ragged)
  clips     2 x 7 x 7 voxels, B = 3: a 128-row tile spans two clips, M = 294 leaves rows past M, the gate rows come from LDS;
            1 x 5 x 8 voxels, B = 4: a tile spans three clips and the gate is read from global memory
  epilogue  with and without residual + ReLU
  layout    the operand's rows are 8 channels wider than cin (ldx > cin)

Every case is forced onto this kernel with the routing knob (conv_route = 3), compared with fp32 torch on the same bf16-rounded
operands under the tolerance of the gated pointwise cases of tests/test_gpu_kernels.py, and compared bit for bit with the kernel
that tests every chunk before loading it (igemm_pw_buf = 0), which is what the layer ran on before.  The padding channels of
the operand hold finite noise; the `poison` cases fill them, and 64 rows behind M, with NaN, so that a load the range check
should have answered shows in the result."""
import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
from gpu_util import _routed_kernel, call, rel_err

pytestmark = pytest.mark.gpu
CANARY, GUARD, PAD, TAIL_ROWS = 7.0, 4096, 8, 64
GEOM = {"two_clips_lds_gate": (3, (2, 7, 7)), "three_clips_global_gate": (4, (1, 5, 8))}


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def generic_kernel_only():
    L.tune(conv_route=3)
    yield
    L.tune(conv_route=0, igemm_pw_buf=1)


def _run(d, y, whole, buf):
    L.tune(igemm_pw_buf=buf)
    whole.fill_(CANARY)
    call("pv_conv3d", d)
    assert _routed_kernel(L.OP_CONV3D, d) == "conv_igemm_kernel"
    n = y.numel()
    assert bool(torch.all(whole[:GUARD] == CANARY)) and bool(torch.all(whole[GUARD + n:] == CANARY)), "write outside the output"
    return y.clone()


def _case(cin, cout, geom, res, poison):
    B, (T, H, W) = GEOM[geom]
    S, ldx = T * H * W, cin + PAD
    fill = float("nan") if poison else 0.0
    # the operand: B * S rows of ldx channels, then TAIL_ROWS rows no voxel owns
    xb = torch.full((B * S + TAIL_ROWS, ldx), fill, dtype=torch.bfloat16)
    if not poison:
        xb[:, cin:] = _rand((B * S + TAIL_ROWS, PAD), 7, 30.0).bfloat16()
        xb[B * S:, :cin] = _rand((TAIL_ROWS, cin), 8, 30.0).bfloat16()
    xb[:B * S, :cin] = _rand((B * S, cin), 1).bfloat16()
    xb = xb.cuda()
    x = xb[:B * S, :cin].view(B, S, cin)
    w = _rand((cout, cin), 2, cin ** -0.5).bfloat16().cuda()
    scale, shift = (_rand((cout,), 3) * 0.2 + 1.0).cuda(), _rand((cout,), 4).cuda()
    g = torch.sigmoid(_rand((B, cin), 5)).cuda()
    r = _rand((B, S, cout), 6).bfloat16().cuda()
    xin = x.float() * g[:, None, :]
    xin = (xin * torch.sigmoid(xin)).bfloat16().float()      # the kernel feeds the MFMA a bf16 operand
    want = F.linear(xin, w.float()) * scale + shift
    if res:
        want = F.relu(want + r.float())
    whole = torch.full((2 * GUARD + B * S * cout,), CANARY, dtype=torch.bfloat16, device="cuda")
    y = whole[GUARD:GUARD + B * S * cout].view(B, S, cout)
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = xb.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.residual, d.a_gate = (r.data_ptr() if res else None), g.data_ptr()
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = S * ldx, S * cout, S * cout, ldx, cout, cout
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin, T, H, W, cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.a_act, d.dtype = (L.ACT_RELU if res else L.ACT_NONE), L.ACT_SWISH, L.PV_BF16
    got = _run(d, y, whole, 1)
    err = rel_err(got, want)
    print("error %.3e" % err)
    assert torch.isfinite(got.float()).all()
    assert err <= 1e-2
    before = _run(d, y, whole, 0)
    assert torch.equal(got.view(torch.int16), before.view(torch.int16)), "differs from the kernel with per-chunk tests"


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res_relu"])
@pytest.mark.parametrize("geom", list(GEOM))
@pytest.mark.parametrize("cout", [192, 200])
@pytest.mark.parametrize("cin", [32, 40, 72, 432])
def test_gated_pointwise_conv_on_the_generic_kernel(generic_kernel_only, cin, cout, geom, res):
    _case(cin, cout, geom, res, poison=False)


@pytest.mark.parametrize("geom", list(GEOM))
@pytest.mark.parametrize("cin,cout", [(40, 200), (432, 192)])
def test_gated_pointwise_conv_with_nan_in_the_padding_and_behind_the_last_row(generic_kernel_only, cin, cout, geom):
    _case(cin, cout, geom, True, poison=True)


def test_ungated_pointwise_conv_on_the_generic_kernel(generic_kernel_only):
    """The path without an operand transform (72 -> 200, three K steps, rows past M, NaN in the padding)."""
    B, S, cin, cout, ldx = 3, 98, 72, 200, 80
    xb = torch.full((B * S + TAIL_ROWS, ldx), float("nan"), dtype=torch.bfloat16)
    xb[:B * S, :cin] = _rand((B * S, cin), 11).bfloat16()
    xb = xb.cuda()
    w = _rand((cout, cin), 12, cin ** -0.5).bfloat16().cuda()
    scale, shift = (_rand((cout,), 13) * 0.2 + 1.0).cuda(), _rand((cout,), 14).cuda()
    want = F.relu(F.linear(xb[:B * S, :cin].float().view(B, S, cin), w.float()) * scale + shift)
    whole = torch.full((2 * GUARD + B * S * cout,), CANARY, dtype=torch.bfloat16, device="cuda")
    y = whole[GUARD:GUARD + B * S * cout].view(B, S, cout)
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = xb.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = S * ldx, S * cout, ldx, cout
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, 2, 7, 7, cin, 2, 7, 7, cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
    got = _run(d, y, whole, 1)
    assert rel_err(got, want) <= 1e-2
    assert torch.equal(got.view(torch.int16), _run(d, y, whole, 0).view(torch.int16))
