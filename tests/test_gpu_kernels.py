"""Kernel-level parity on the MI355X: each C-ABI entry point against a plain PyTorch fp32
reference of the same op on the same seeded inputs, including ragged / odd sizes.

Tolerances (relative to the reference abs-max): fp32 kernels 1e-3 (in practice ~1e-6), bf16
kernels 1e-2 against the fp32 reference evaluated on the same bf16-rounded inputs.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
from gpu_util import _routed_kernel, call, pv_dtype, rel_err

pytestmark = pytest.mark.gpu
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


def _rand(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).cuda()


def _attention_ref(q, k, v, heads, scale, residual_q):
    B, Nq, Cw = q.shape
    hd = Cw // heads
    qh = q.float().reshape(B, Nq, heads, hd).permute(0, 2, 1, 3)
    kh = k.float().reshape(B, -1, heads, hd).permute(0, 2, 1, 3)
    vh = v.float().reshape(B, -1, heads, hd).permute(0, 2, 1, 3)
    a = torch.softmax((qh * scale) @ kh.transpose(-2, -1), dim=-1)
    o = a @ vh
    if residual_q:
        o = o + qh
    return o.permute(0, 2, 1, 3).reshape(B, Nq, Cw)


def _run_attention(q, k, v, heads, scale, residual_q, pad=0, routed=None):
    """q/k/v: (B, N, heads*hd) device tensors, possibly channel slices of a wider buffer.  routed: a list that receives the
    symbol of the kernel the descriptor is routed to under the current knobs."""
    B, Nq, Cw = q.shape
    o = torch.full((B, Nq, Cw + pad), 7.0, dtype=q.dtype, device="cuda")
    d = L.AttentionDesc()
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.q_bs, d.k_bs, d.v_bs, d.o_bs = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(1), k.stride(1), v.stride(1), o.stride(1)
    d.B, d.heads, d.head_dim, d.Nq, d.Nk = B, heads, Cw // heads, Nq, k.shape[1]
    d.scale, d.residual_q, d.dtype = scale, int(residual_q), pv_dtype(q)
    call("pv_attention", d)
    if routed is not None:
        routed.append(_routed_kernel(L.OP_ATTENTION, d))
    if pad:
        assert torch.all(o[:, :, Cw:] == 7.0)  # never writes outside its channels
    return o[:, :, :Cw]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,heads,hd,Nq,Nk,res", [
    (2, 2, 96, 785, 785, False),     # MViT-B block 15 geometry
    (1, 1, 96, 1000, 197, False),    # many q blocks, ragged key tail
    (2, 4, 96, 129, 65, True),       # one row past a q block / one key past a tile, residual_pool
    (1, 8, 96, 33, 3137, False),     # long key loop
    (3, 1, 32, 7, 5, False),         # smaller than one tile
    (1, 2, 64, 200, 130, True),
    (1, 1, 128, 140, 70, False),
    (1, 2, 96, 70, 64, False),       # exactly one full key tile (pipelined kernel: prologue + last step only)
    (1, 1, 96, 130, 128, True),      # two full tiles: nothing to mask in the last one
    (2, 1, 64, 40, 192, False),      # three full tiles, odd tile count
    (1, 1, 32, 300, 256, False),     # four full tiles, head_dim 32 (side work spread over 4 PV MFMAs)
])
def test_attention_matches_reference(dtype, B, heads, hd, Nq, Nk, res):
    Cw = heads * hd
    q, k, v = _rand((B, Nq, Cw), 1, dtype), _rand((B, Nk, Cw), 2, dtype), _rand((B, Nk, Cw), 3, dtype)
    scale = hd ** -0.5
    want = _attention_ref(q, k, v, heads, scale, res)
    got = _run_attention(q, k, v, heads, scale, res, pad=8)
    assert rel_err(got, want) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,heads,Nq,Nk", [
    (1, 1, 50177, 785),     # MViT-B 32x3 block 0 (hub/vision_transformers.py:31-39): 16*56*56+1 queries x 16*7*7+1 keys
    (2, 2, 12545, 3137),    # block 1: 16*28*28+1 queries x 16*14*14+1 keys
    (1, 4, 3137, 3137),     # block 3
    (1, 8, 785, 3137),      # block 14
])
def test_attention_at_the_mvit_b_32x3_geometries(dtype, B, heads, Nq, Nk):
    """The (Nq, Nk, heads) of MViT-B 32x3 at 224^2, head_dim 96, reference in chunks of queries."""
    hd = 96
    Cw = heads * hd
    q, k, v = _rand((B, Nq, Cw), 31, dtype), _rand((B, Nk, Cw), 32, dtype), _rand((B, Nk, Cw), 33, dtype)
    scale = hd ** -0.5
    got = _run_attention(q, k, v, heads, scale, False)
    worst, amax = 0.0, 0.0
    for lo in range(0, Nq, 4096):
        want = _attention_ref(q[:, lo:lo + 4096], k, v, heads, scale, False)
        worst = max(worst, (got[:, lo:lo + 4096].float() - want).abs().max().item())
        amax = max(amax, want.abs().max().item())
    assert worst / amax <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_on_channel_slices_of_a_fused_qkv_buffer(dtype):
    B, heads, hd, N = 2, 2, 96, 300
    Cw = heads * hd
    qkv = _rand((B, N, 3 * Cw), 5, dtype)
    q, k, v = qkv[:, :, :Cw], qkv[:, :, Cw:2 * Cw], qkv[:, :, 2 * Cw:]
    want = _attention_ref(q, k, v, heads, hd ** -0.5, False)
    got = _run_attention(q, k, v, heads, hd ** -0.5, False)
    assert rel_err(got, want) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_online_softmax_rescale_branch(dtype):
    """A key late in the sequence dominates one query: the running max jumps by ~60 in the
    exp2 domain at a chosen tile, so every earlier tile's contribution must be rescaled away."""
    B, heads, hd, Nq, Nk = 1, 1, 96, 64, 400
    q, k, v = _rand((B, Nq, hd), 11, dtype, 0.5), _rand((B, Nk, hd), 12, dtype, 0.5), _rand((B, Nk, hd), 13, dtype)
    k[0, 333] = (q[0, 17].float() * 8.0).to(dtype)   # spike: score(q17, k333) >> all others
    k[0, 2] = (q[0, 40].float() * 8.0).to(dtype)     # and one in the very first tile
    want = _attention_ref(q, k, v, heads, hd ** -0.5, False)
    got = _run_attention(q, k, v, heads, hd ** -0.5, False)
    assert rel_err(got, want) <= TOL[dtype]
    assert rel_err(got[0, 17], v[0, 333].float()) <= 2e-2  # the spiked row is (almost) a copy of v[333]


@pytest.mark.parametrize("hd", [96, 64, 32])
@pytest.mark.parametrize("B,heads,Nq,Nk,res", [
    (2, 2, 785, 785, True),       # MViT-B block 15, residual_pool
    (1, 1, 1000, 197, False),     # ragged key tail, several workgroups
    (2, 4, 129, 65, True),        # one row past a 32-row block / one key past a tile
    (1, 2, 300, 64, False),       # exactly one key tile: prologue + last step only
    (1, 1, 130, 128, True),       # two full tiles
    (1, 3, 257, 192, False),      # three full tiles (odd count), one row past two 128-row items
    (1, 1, 40, 384, True),        # six full tiles: the pipelined steps on both parities
    (1, 8, 33, 3137, False),      # long key loop
    (2, 1, 3137, 785, True),      # MViT-B blocks 4-13 (one head of it)
])
def test_attention_every_kernel_form_of_head_dim_96(hd, B, heads, Nq, Nk, res):
    """The two pipelined bf16 kernels at the tile counts their steps distinguish, against the fp32 reference
    (layers/attention.py:531-539): pv_attention routes head_dim 96 (MViT) to attn_w64_kernel (pv_attn64.hip) and head_dim
    64 / 32 to attn_pipe_kernel (pv_attn.hip); the route is asserted, no knob is involved."""
    dtype = torch.bfloat16
    Cw = heads * hd
    q, k, v = _rand((B, Nq, Cw), 41, dtype), _rand((B, Nk, Cw), 42, dtype), _rand((B, Nk, Cw), 43, dtype)
    want = _attention_ref(q, k, v, heads, hd ** -0.5, res)
    routed = []
    got = _run_attention(q, k, v, heads, hd ** -0.5, res, pad=8, routed=routed)
    assert rel_err(got, want) <= TOL[dtype]
    assert routed[0] == ("attn_w64_kernel" if hd == 96 else "attn_pipe_kernel"), routed


@pytest.mark.parametrize("hd", [96, 64])
def test_attention_forms_take_the_rescale_branch_and_a_masked_first_tile(hd):
    """The rescale block of attn_w64_kernel (head_dim 96) and of attn_pipe_kernel (head_dim 64), and their ragged single-tile
    path: a spiked key late in the sequence, one in the very first tile, and Nk < 64."""
    B, heads, Nq, Nk = 1, 1, 64, 400
    dtype = torch.bfloat16
    q, k, v = _rand((B, Nq, hd), 11, dtype, 0.5), _rand((B, Nk, hd), 12, dtype, 0.5), _rand((B, Nk, hd), 13, dtype)
    k[0, 333] = (q[0, 17].float() * 8.0).to(dtype)
    k[0, 2] = (q[0, 40].float() * 8.0).to(dtype)
    k[0, 130] = (q[0, 50].float() * 6.0).to(dtype)    # row 50 (another wave's 32-row block) grows at another tile
    want = _attention_ref(q, k, v, heads, hd ** -0.5, False)
    got = _run_attention(q, k, v, heads, hd ** -0.5, False)
    small = _run_attention(q[:, :, :], k[:, :37], v[:, :37], heads, hd ** -0.5, True)
    assert rel_err(got, want) <= TOL[dtype]
    assert rel_err(got[0, 17], v[0, 333].float()) <= 2e-2
    assert rel_err(small, _attention_ref(q, k[:, :37], v[:, :37], heads, hd ** -0.5, True)) <= TOL[dtype]


def test_attention_rejects_bad_descriptors():
    lib = L.lib()
    d = L.AttentionDesc()
    assert lib.pv_attention(C.byref(d), None) == L.PV_ERR_INVALID
    q = torch.zeros(1, 8, 40, device="cuda")
    d.q = d.k = d.v = d.o = q.data_ptr()
    d.B, d.heads, d.head_dim, d.Nq, d.Nk = 1, 1, 40, 8, 8
    d.ldq = d.ldk = d.ldv = d.ldo = 40
    d.q_bs = d.k_bs = d.v_bs = d.o_bs = 320
    d.dtype = L.PV_F32
    d.scale = 1.0
    assert lib.pv_attention(C.byref(d), None) == L.PV_ERR_UNSUPPORTED  # head_dim 40
    # scale must be finite and > 0 (the kernels take row maxima before scaling), whichever kernel the descriptor routes to
    qb, ob = torch.zeros(1, 8, 32, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 8, 32, dtype=torch.bfloat16, device="cuda")
    d = L.AttentionDesc()
    d.q = d.k = d.v = qb.data_ptr()
    d.o = ob.data_ptr()
    d.B, d.heads, d.head_dim, d.Nq, d.Nk = 1, 1, 32, 8, 8
    d.ldq = d.ldk = d.ldv = d.ldo = 32
    d.q_bs = d.k_bs = d.v_bs = d.o_bs = 256
    d.dtype = L.PV_BF16
    for bad in (0.0, -0.125, float("inf"), float("nan")):
        d.scale = bad
        assert lib.pv_attention(C.byref(d), None) == L.PV_ERR_INVALID, bad
    d.scale = 0.125
    assert lib.pv_attention(C.byref(d), None) == L.PV_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------ depthwise conv on tokens
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("heads,thw,stride,cls", [
    (2, (4, 14, 14), (1, 2, 2), 1), (1, (2, 16, 16), (1, 8, 8), 1), (4, (4, 7, 7), (1, 1, 1), 1),
    (2, (4, 8, 8), (2, 2, 2), 0),
])
def test_token_pooling_conv_with_shared_weights_and_cls_prefix(dtype, heads, thw, stride, cls):
    """MViT's pool_q/k/v (layers/attention.py:185-200): depthwise 3x3x3 conv over the token grid,
    weights shared across heads, cls row copied through."""
    hd, B = 96, 2
    T, H, W = thw
    Cw = heads * hd
    x = _rand((B, cls + T * H * W, Cw), 21, dtype)
    w = _rand((hd, 1, 3, 3, 3), 22, torch.float32, 0.3)
    grid = x[:, cls:].float().reshape(B, T, H, W, heads, hd).permute(0, 4, 5, 1, 2, 3).reshape(B * heads, hd, T, H, W)
    ref = F.conv3d(grid, w, None, stride=stride, padding=1, groups=hd)
    To, Ho, Wo = ref.shape[2:]
    ref = ref.reshape(B, heads, hd, To * Ho * Wo).permute(0, 3, 1, 2).reshape(B, To * Ho * Wo, Cw)
    if cls:
        ref = torch.cat([x[:, :1].float(), ref], 1)
    y = torch.zeros(B, cls + To * Ho * Wo, Cw, dtype=dtype, device="cuda")
    wp = w.reshape(hd, 27).t().contiguous()
    d = L.DwConv3dDesc()
    d.x, d.w, d.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = x.stride(0), y.stride(0), Cw, Cw
    d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = B, T, H, W, Cw, To, Ho, Wo
    d.kt = d.kh = d.kw = 3
    d.st, d.sh, d.sw = stride
    d.pt = d.ph = d.pw = 1
    d.w_mod, d.act, d.dtype, d.n_prefix = (hd if heads > 1 else 0), L.ACT_NONE, pv_dtype(x), cls
    call("pv_dwconv3d", d)
    assert rel_err(y, ref) <= TOL[dtype]


# ------------------------------------------------------------------ row ops
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,Cc", [(1000, 96), (77, 768), (5, 1536), (130, 192)])
def test_layernorm_rows(dtype, rows, Cc):
    x = _rand((rows, Cc), 31, dtype, 2.0) + 0.5
    g, b = _rand((Cc,), 32, torch.float32), _rand((Cc,), 33, torch.float32)
    want = F.layer_norm(x.float(), (Cc,), g, b, 1e-6)
    y = torch.zeros_like(x)
    d = L.RowsDesc()
    d.x, d.y, d.gamma, d.beta = x.data_ptr(), y.data_ptr(), g.data_ptr(), b.data_ptr()
    d.rows, d.C, d.ldx, d.ldy, d.eps, d.dtype = rows, Cc, Cc, Cc, 1e-6, pv_dtype(x)
    call("pv_layernorm", d)
    assert rel_err(y, want) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tokens,heads,hd", [(785, 4, 96), (50, 8, 96), (333, 1, 64), (77, 2, 128)])
def test_layernorm_per_head_with_periodic_parameter_table(dtype, tokens, heads, hd):
    """LayerNorm(head_dim) over k|v packed side by side (2*heads rows of `hd` per token), the first
    `heads` rows of every token normalised with pool_k's parameters, the rest with pool_v's."""
    P = 2 * heads
    x = _rand((tokens, P, hd), 131, dtype, 2.0) + 0.25
    gk, bk = _rand((hd,), 132, torch.float32), _rand((hd,), 133, torch.float32)
    gv, bv = _rand((hd,), 134, torch.float32), _rand((hd,), 135, torch.float32)
    want = torch.cat([F.layer_norm(x[:, :heads].float(), (hd,), gk, bk, 1e-6),
                      F.layer_norm(x[:, heads:].float(), (hd,), gv, bv, 1e-6)], 1)
    gam = torch.cat([gk.repeat(heads), gv.repeat(heads)]).contiguous()
    bet = torch.cat([bk.repeat(heads), bv.repeat(heads)]).contiguous()
    y = torch.zeros_like(x)
    d = L.RowsDesc()
    d.x, d.y, d.gamma, d.beta = x.data_ptr(), y.data_ptr(), gam.data_ptr(), bet.data_ptr()
    d.rows, d.C, d.ldx, d.ldy, d.eps, d.dtype, d.g_period = tokens * P, hd, hd, hd, 1e-6, pv_dtype(x), P
    call("pv_layernorm", d)
    assert rel_err(y, want) <= TOL[dtype]


# ------------------------------------------------------------------ GEMM (linear) shapes of MViT
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,K,N,act,res", [
    (785 * 2, 768, 3072, L.ACT_GELU, False), (3137, 384, 1152, L.ACT_NONE, False),
    (1001, 96, 288, L.ACT_NONE, True), (785, 3072, 768, L.ACT_NONE, True), (50, 768, 400, L.ACT_NONE, False),
    (333, 96, 80, L.ACT_SIGMOID, False), (77, 2048, 80, L.ACT_SIGMOID, False),    # multi-label heads: streaming / LDS-DMA kernel
])
def test_linear_as_pointwise_conv(dtype, M, K, N, act, res):
    x = _rand((1, M, K), 41, dtype)
    w = _rand((N, K), 42, dtype, K ** -0.5)
    bias = _rand((N,), 43, torch.float32)
    r = _rand((1, M, N), 44, dtype) if res else None
    want = F.linear(x.float(), w.float(), bias)
    if res:
        want = want + r.float()
    if act == L.ACT_GELU:
        want = F.gelu(want)
    if act == L.ACT_SIGMOID:
        want = torch.sigmoid(want)
    y = torch.zeros(1, M, N, dtype=dtype, device="cuda")
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), bias.data_ptr()
    d.residual = r.data_ptr() if res else None
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = M * K, M * N, M * N, K, N, N
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = 1, 1, 1, M, K, 1, 1, M, N
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.a_act, d.dtype, d.y_f32 = act, L.ACT_NONE, pv_dtype(x), 0
    call("pv_conv3d", d)
    assert rel_err(y, want) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,k,dil,stride", [
    (64, 64, (1, 3, 3), (1, 2, 2), (1, 1, 1)),      # slow_r50_detection res5 conv_b (LDS-DMA GEMM kernel in bf16)
    (16, 24, (3, 3, 3), (2, 1, 3), (1, 2, 1)),      # generic kernel, dilation on T and W, stride on H
    (128, 96, (3, 1, 1), (2, 1, 1), (1, 1, 1)),     # temporal taps two frames apart
])
def test_dilated_dense_conv(dtype, cin, cout, k, dil, stride):
    """nn.Conv3d(dilation=...) as create_resnet's stage_conv_b_dilation builds it (models/resnet.py:780-791)."""
    B, T, H, W = 2, 5, 11, 13
    pad = tuple(d * (kk // 2) for d, kk in zip(dil, k))
    x = _rand((B, T, H, W, cin), 151, dtype)
    w = _rand((cout, cin) + k, 152, dtype, (cin * k[0] * k[1] * k[2]) ** -0.5)
    bias = _rand((cout,), 153, torch.float32)
    want = F.relu(F.conv3d(x.float().permute(0, 4, 1, 2, 3), w.float(), bias, stride=stride, padding=pad, dilation=dil))
    To, Ho, Wo = want.shape[2:]
    y = torch.full((B, To, Ho, Wo, cout), 5.0, dtype=dtype, device="cuda")
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.shift = x.data_ptr(), wp.data_ptr(), y.data_ptr(), bias.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin, To * Ho * Wo * cout, cin, cout
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin, To, Ho, Wo, cout
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *stride, *pad)
    d.dil_t, d.dil_h, d.dil_w = dil
    d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, pv_dtype(x)
    call("pv_conv3d", d)
    assert rel_err(y.permute(0, 4, 1, 2, 3), want) <= TOL[dtype]
    d.To += 1     # the output size nn.Conv3d would NOT produce is refused
    assert L.lib().pv_conv3d(C.byref(d), None) == L.PV_ERR_INVALID


# ------------------------------------------------------------------ X3D pointwise convs (streaming kernel)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,K,N,gate,res", [
    (2, 3136, 24, 54, False, False),    # conv_a res2
    (3, 784, 54, 24, True, True),       # conv_c res2 with SE gate + swish on load + residual
    (2, 100, 108, 48, True, True),      # S not a multiple of 16: wave tiles straddle clips
    (2, 196, 216, 96, True, True), (1, 200, 96, 216, False, False), (2, 49, 192, 432, False, False),
    (2, 80, 432, 192, True, True),      # K too large for the streaming kernel -> generic path
])
def test_pointwise_conv_with_se_gate_swish_and_residual(dtype, B, S, K, N, gate, res):
    Kp, Np = (K + 7) // 8 * 8, (N + 7) // 8 * 8
    x = torch.zeros(B, S, Kp, dtype=dtype, device="cuda")
    x[:, :, :K] = _rand((B, S, K), 51, dtype)
    w = torch.zeros(N, Kp, dtype=dtype, device="cuda")
    w[:, :K] = _rand((N, K), 52, dtype, K ** -0.5)
    scale, shift = _rand((N,), 53, torch.float32) * 0.2 + 1.0, _rand((N,), 54, torch.float32)
    g = torch.zeros(B, Kp, dtype=torch.float32, device="cuda")
    g[:, :K] = torch.sigmoid(_rand((B, K), 55, torch.float32))
    r = torch.zeros(B, S, Np, dtype=dtype, device="cuda")
    r[:, :, :N] = _rand((B, S, N), 56, dtype)
    xin = x.float()[:, :, :K]
    if gate:
        xin = xin * g[:, None, :K]
        xin = xin * torch.sigmoid(xin)
        if dtype == torch.bfloat16:
            xin = xin.bfloat16().float()   # the kernel feeds the MFMA a bf16 operand
    want = F.linear(xin, w.float()[:, :K]) * scale + shift
    if res:
        want = want + r.float()[:, :, :N]
    want = F.relu(want)
    y = torch.full((B, S, Np), 3.0, dtype=dtype, device="cuda")
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.residual = r.data_ptr() if res else None
    d.a_gate = g.data_ptr() if gate else None
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = S * Kp, S * Np, S * Np, Kp, Np, Np
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, 1, 1, S, Kp, 1, 1, S, N
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.a_act, d.dtype = L.ACT_RELU, (L.ACT_SWISH if gate else L.ACT_NONE), pv_dtype(x)
    call("pv_conv3d", d)
    assert rel_err(y[:, :, :N], want) <= TOL[dtype]
    assert torch.all(y[:, :, N:] == 0)   # padding channels are written as exact zeros


# ------------------------------------------------------------------ first-layer conv on the 4-channel layout
_C4_CASES = [   # B, T, H, W, cout, k, s, p, f32out, pos, kernel the library routes it to
    (2, 4, 32, 32, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), False, None, "stem7_kernel"),    # SlowFast slow stem
    (1, 8, 24, 40, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3), False, None, "stem7_kernel"),     # SlowFast fast stem
    (2, 4, 18, 22, 24, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, None, "stem_c4_kernel"),  # X3D stem conv (odd kw: padded pair)
    (1, 6, 28, 28, 96, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, None, "stem_pe_kernel"),   # MViT patch embedding (+bias, fp32 out)
    (1, 3, 9, 11, 20, (3, 2, 4), (1, 1, 3), (1, 0, 2), False, None, "stem_c4_kernel"),   # odd everything
    # 7x7 / stride 2 with the input tile staged in LDS (stem7_kernel): several ragged tiles, frame ring wrapping
    (1, 9, 70, 150, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), False, None, "stem7_kernel"),
    (2, 9, 50, 134, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3), False, None, "stem7_kernel"),
    (1, 5, 40, 70, 32, (3, 7, 7), (1, 2, 2), (1, 3, 3), False, None, "stem7_kernel"),
    (1, 3, 21, 37, 6, (7, 7, 7), (1, 2, 2), (3, 3, 3), False, None, "stem7_kernel"),
    (1, 2, 33, 66, 16, (1, 7, 7), (1, 2, 2), (0, 3, 3), False, None, "stem7_kernel"),
    # MViT patch embedding geometries on stem_pe_kernel (filter in registers across the waves, input tile in LDS)
    (2, 5, 30, 50, 96, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, None, "stem_pe_kernel"),      # ragged tiles, odd T
    (1, 1, 64, 64, 96, (1, 7, 7), (1, 4, 4), (0, 3, 3), True, None, "stem_pe_kernel"),      # mvit_base_16: the image model's Conv2d as one frame
    (1, 4, 36, 68, 64, (3, 7, 7), (2, 4, 4), (1, 3, 3), False, None, "stem_pe_kernel"),     # 4 waves, bf16 out
    (1, 3, 40, 40, 120, (3, 7, 7), (1, 4, 4), (1, 3, 3), True, None, "stem_pe_kernel"),     # 8 waves, channel tail, temporal stride 1
    # the generic kernel on 7x7 convs the tiled kernels do not take: 40 channels are neither <= 8 nor a multiple of 16
    # (stem_c4_kernel<4, 2>); 76 channels = 5 tiles are no stem_pe width (stem_c4_kernel<2, 2>: three blockIdx.y slabs,
    # channel tail inside the last one)
    (1, 2, 18, 22, 40, (1, 7, 7), (1, 2, 2), (0, 3, 3), False, None, "stem_c4_kernel"),
    (1, 3, 20, 28, 76, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, None, "stem_c4_kernel"),
    # position tables added in the fp32 epilogue: spatial [Ho*Wo, cout] + temporal [To, cout], or one full [To*Ho*Wo, cout]
    (1, 3, 20, 28, 76, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, "split", "stem_c4_kernel"),
    (1, 3, 20, 28, 76, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, "full", "stem_c4_kernel"),
    (2, 5, 30, 50, 96, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, "split", "stem_pe_kernel"),
    (2, 5, 30, 50, 96, (3, 7, 7), (2, 4, 4), (1, 3, 3), True, "full", "stem_pe_kernel"),
]


def _c4_case_id(i, c):
    """The id pytest gave case i before `pos` and `kern` were parameters (so the earlier cases keep their names), plus pos."""
    base = "-".join(str(v) for v in c[:5]) + "-k%d-s%d-p%d-%s" % (i, i, i, c[8])
    return base if c[9] is None else base + "-" + c[9]


@pytest.mark.parametrize("B,T,H,W,cout,k,s,p,f32out,pos,kern", _C4_CASES,
                         ids=[_c4_case_id(i, c) for i, c in enumerate(_C4_CASES)])
def test_first_layer_conv_on_c4_layout(B, T, H, W, cout, k, s, p, f32out, pos, kern):
    x = _rand((B, 3, T, H, W), 61, torch.bfloat16)
    w = _rand((cout, 3) + k, 62, torch.bfloat16, (3 * k[0] * k[1] * k[2]) ** -0.5)
    bias = _rand((cout,), 63, torch.float32)
    want = F.relu(F.conv3d(x.float(), w.float(), bias, stride=s, padding=p))
    To, Ho, Wo = want.shape[2:]
    pos_s = pos_t = None
    if pos == "split":
        pos_s, pos_t = _rand((Ho * Wo, cout), 64, torch.float32), _rand((To, cout), 65, torch.float32)
        want = want + (pos_t[:, None, :] + pos_s[None, :, :]).reshape(To, Ho, Wo, cout).permute(3, 0, 1, 2)
    elif pos == "full":
        pos_s = _rand((To * Ho * Wo, cout), 64, torch.float32)
        want = want + pos_s.reshape(To, Ho, Wo, cout).permute(3, 0, 1, 2)
    # NCDHW -> NDHWC with 4 channels per voxel, through the library's own ingest
    x4 = torch.full((B, T, H, W, 4), 9.0, dtype=torch.bfloat16, device="cuda")
    ld = L.LayoutDesc()
    ld.src, ld.dst = x.data_ptr(), x4.data_ptr()
    ld.B, ld.C, ld.T, ld.H, ld.W, ld.c_p, ld.ld, ld.bs = B, 3, T, H, W, 4, 4, T * H * W * 4
    ld.src_dtype, ld.dst_dtype = L.PV_BF16, L.PV_BF16
    call("pv_ingest_ncdhw", ld)
    assert torch.equal(x4[..., :3].permute(0, 4, 1, 2, 3), x) and torch.all(x4[..., 3] == 0)
    kwp = (k[2] + 1) // 2 * 2
    wp = torch.zeros(cout, k[0], k[1], kwp, 4, dtype=torch.bfloat16, device="cuda")
    wp[:, :, :, : k[2], :3] = w.permute(0, 2, 3, 4, 1)
    cp = (cout + 7) // 8 * 8
    y = torch.full((B, To, Ho, Wo, cp), 5.0, dtype=torch.float32 if f32out else torch.bfloat16, device="cuda")
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.shift = x4.data_ptr(), wp.data_ptr(), y.data_ptr(), bias.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * 4, To * Ho * Wo * cp, 4, cp
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, 4, To, Ho, Wo, cout
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *s, *p)
    d.act, d.a_act, d.dtype, d.y_f32 = L.ACT_RELU, L.ACT_NONE, L.PV_BF16, int(f32out)
    d.pos_spatial = pos_s.data_ptr() if pos_s is not None else None
    d.pos_temporal = pos_t.data_ptr() if pos_t is not None else None
    call("pv_conv3d", d)
    assert rel_err(y[..., :cout].permute(0, 4, 1, 2, 3), want) <= (2e-3 if f32out else 1e-2)
    assert torch.all(y[..., cout:] == 0)
    assert _routed_kernel(L.OP_CONV3D, d) == kern


@pytest.mark.parametrize("B,T,H,W,cout,k,s,p", [
    (1, 8, 24, 40, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3)),     # SlowFast fast stem
    (2, 3, 17, 23, 8, (1, 7, 7), (1, 2, 2), (0, 3, 3)),     # odd output width: the last column holds one output
    (1, 4, 12, 15, 5, (3, 3, 3), (1, 1, 1), (1, 1, 1)),     # stride 1, fewer than 8 channels
    (1, 2, 10, 31, 8, (1, 5, 4), (1, 2, 3), (0, 2, 1)),     # even kernel width, stride 3
])
def test_first_layer_conv_two_outputs_per_mfma_column(B, T, H, W, cout, k, s, p):
    """c4_wpair = 2 (csrc/pv_stem.hip): same result as the plain first-layer conv and as torch."""
    x = _rand((B, 3, T, H, W), 141, torch.bfloat16)
    w = _rand((cout, 3) + k, 142, torch.bfloat16, (3 * k[0] * k[1] * k[2]) ** -0.5)
    bias = _rand((cout,), 143, torch.float32)
    want = F.relu(F.conv3d(x.float(), w.float(), bias, stride=s, padding=p))
    To, Ho, Wo = want.shape[2:]
    x4 = torch.zeros(B, T, H, W, 4, dtype=torch.bfloat16, device="cuda")
    x4[..., :3] = x.permute(0, 2, 3, 4, 1)
    kwp = (k[2] + s[2] + 1) // 2 * 2
    wp = torch.zeros(2, 8, k[0], k[1], kwp, 4, dtype=torch.bfloat16, device="cuda")
    for j in range(2):
        wp[j, :cout, :, :, j * s[2]: j * s[2] + k[2], :3] = w.permute(0, 2, 3, 4, 1)
    y = torch.full((B, To, Ho, Wo, 8), 5.0, dtype=torch.bfloat16, device="cuda")
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.shift = x4.data_ptr(), wp.data_ptr(), y.data_ptr(), bias.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * 4, To * Ho * Wo * 8, 4, 8
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, 4, To, Ho, Wo, cout
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *s, *p)
    d.act, d.a_act, d.dtype, d.c4_wpair = L.ACT_RELU, L.ACT_NONE, L.PV_BF16, 2
    call("pv_conv3d", d)
    assert rel_err(y[..., :cout].permute(0, 4, 1, 2, 3), want) <= 1e-2
    assert torch.all(y[..., cout:] == 0)


@pytest.mark.parametrize("mode", ["block_norm", "pre_pool", "copy_rows"])
def test_affine_rows_is_batchnorm_eval_on_tokens(mode):
    """pv_affine_rows: nn.BatchNorm1d block norms (fp32 stream -> bf16 operand), nn.BatchNorm3d(head_dim) + GELU before
    the pooling conv in place on a column slice with the cls rows untouched (reference layers/attention.py:186-190,
    738-753), and the plain fp32 -> bf16 row copy used for the cls rows of a head without a final norm."""
    B, N, Cn = 3, 37, 88
    g, b = _rand((Cn,), 311, torch.float32) * 0.3 + 1.0, _rand((Cn,), 312, torch.float32) * 0.4
    d = L.RowsDesc()
    if mode == "block_norm":
        x = _rand((B, N, Cn), 313, torch.float32)
        y = torch.full((B, N, Cn), 7.0, dtype=torch.bfloat16, device="cuda")
        want = x * g + b
        d.x, d.y, d.gamma, d.beta = x.data_ptr(), y.data_ptr(), g.data_ptr(), b.data_ptr()
        d.rows, d.C, d.ldx, d.ldy, d.dtype, d.x_f32 = B * N, Cn, Cn, Cn, L.PV_BF16, 1
        call("pv_affine_rows", d)
        assert rel_err(y.float(), want) <= 4e-3
    elif mode == "pre_pool":
        ld = 3 * Cn                                   # the k slice of a qkv GEMM output
        buf = _rand((B, N, ld), 314, torch.bfloat16)
        before = buf.clone()
        want = F.gelu(before[:, :, Cn:2 * Cn].float() * g + b)
        d.x = d.y = buf.data_ptr() + Cn * 2
        d.gamma, d.beta = g.data_ptr(), b.data_ptr()
        d.rows, d.C, d.ldx, d.ldy, d.dtype = B * N, Cn, ld, ld, L.PV_BF16
        d.rows_per_batch, d.n_prefix, d.act = N, 1, L.ACT_GELU
        call("pv_affine_rows", d)
        assert rel_err(buf[:, 1:, Cn:2 * Cn].float(), want[:, 1:]) <= 8e-3
        assert torch.equal(buf[:, 0], before[:, 0])                                   # cls rows untouched
        assert torch.equal(buf[:, :, :Cn], before[:, :, :Cn]) and torch.equal(buf[:, :, 2 * Cn:], before[:, :, 2 * Cn:])
    else:
        x = _rand((B, N, Cn), 315, torch.float32)     # row 0 of every batch item -> dense [B, C]
        y = torch.full((B, Cn), 7.0, dtype=torch.bfloat16, device="cuda")
        d.x, d.y = x.data_ptr(), y.data_ptr()
        d.rows, d.C, d.ldx, d.ldy, d.dtype, d.x_f32 = B, Cn, N * Cn, Cn, L.PV_BF16, 1
        call("pv_affine_rows", d)
        assert torch.equal(y, x[:, 0].bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,H,W,Cn,gw,k,s,p", [
    (2, 4, 9, 11, 32, 4, (3, 3, 3), (1, 1, 1), (1, 1, 1)),     # create_csn(stage_conv_b_width_per_group=4)
    (1, 3, 10, 7, 24, 2, (3, 3, 3), (1, 2, 2), (1, 1, 1)),     # strided, Cn not a multiple of 16
    (1, 5, 6, 6, 40, 8, (3, 1, 1), (2, 1, 1), (1, 0, 0)),      # whole 8-channel chunks per group, temporal stride
])
def test_channelwise_grouped_conv(B, T, H, W, Cn, gw, k, s, p, dtype):
    """pv_dwconv3d with gw input channels per output channel = nn.Conv3d(C, C, groups=C // gw) + BN + ReLU
    (reference models/csn.py:34,169: conv_b_num_groups = dim_inner // stage_conv_b_width_per_group)."""
    x = _rand((B, Cn, T, H, W), 301, dtype)
    w = _rand((Cn, gw) + k, 302, torch.float32, (gw * k[0] * k[1] * k[2]) ** -0.5)
    scale, shift = _rand((Cn,), 303, torch.float32) * 0.2 + 1.0, _rand((Cn,), 304, torch.float32) * 0.5
    want = F.conv3d(x.float(), w, None, stride=s, padding=p, groups=Cn // gw)
    want = F.relu(want * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    To, Ho, Wo = want.shape[2:]
    cp = (Cn + 7) // 8 * 8
    xl = torch.zeros(B, T, H, W, cp, dtype=dtype, device="cuda")
    xl[..., :Cn] = x.permute(0, 2, 3, 4, 1)
    taps = k[0] * k[1] * k[2]
    wp = torch.zeros(taps, gw, cp, dtype=torch.float32, device="cuda")
    wp[:, :, :Cn] = w.reshape(Cn, gw, taps).permute(2, 1, 0)
    y = torch.full((B, To, Ho, Wo, cp), 5.0, dtype=dtype, device="cuda")
    d = L.DwConv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = xl.data_ptr(), wp.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cp, To * Ho * Wo * cp, cp, cp
    d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = B, T, H, W, Cn, To, Ho, Wo
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *s, *p)
    d.act, d.dtype, d.gw = L.ACT_RELU, L.PV_F32 if dtype == torch.float32 else L.PV_BF16, gw
    call("pv_dwconv3d", d)
    assert rel_err(y[..., :Cn].permute(0, 4, 1, 2, 3).float(), want) <= (1e-5 if dtype == torch.float32 else 1e-2)
    assert torch.all(y[..., Cn:] == 0)
    d.gw = 3                                        # only 2 / 4 / 8 channels per group
    assert L.lib().pv_dwconv3d(C.byref(d), None) == L.PV_ERR_UNSUPPORTED


@pytest.mark.parametrize("B,T,H,W,cout,dk,act", [
    (2, 16, 30, 34, 24, 5, L.ACT_RELU),   # X3D stem: 1x3x3 s(1,2,2) 3->24, then depthwise 5x1x1, BN, ReLU
    (1, 4, 18, 22, 24, 5, L.ACT_RELU),    # clip shorter than one unrolled ring turn
    (3, 7, 9, 70, 20, 3, L.ACT_NONE),     # 3 temporal taps, T not a multiple of anything, ragged voxel tiles
])
def test_x3d_stem_conv_xy_and_temporal_depthwise_in_one_launch(B, T, H, W, cout, dk, act):
    """models/x3d.py:66-88: Conv2plus1d(conv_xy -> conv_t depthwise, nothing in between) + norm + act."""
    x = _rand((B, 3, T, H, W), 71, torch.bfloat16)
    w = _rand((cout, 3, 1, 3, 3), 72, torch.bfloat16, 27 ** -0.5)
    wt = _rand((cout, 1, dk, 1, 1), 73, torch.float32, 0.5)
    scale, shift = _rand((cout,), 74, torch.float32) * 0.2 + 1.0, _rand((cout,), 75, torch.float32) * 0.5
    h = F.conv3d(x.float(), w.float(), None, stride=(1, 2, 2), padding=(0, 1, 1))
    pre = F.conv3d(h, wt, None, padding=(dk // 2, 0, 0), groups=cout)
    pre = pre * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    want = F.relu(pre) if act == L.ACT_RELU else pre
    To, Ho, Wo = want.shape[2:]
    x4 = torch.zeros(B, T, H, W, 4, dtype=torch.bfloat16, device="cuda")
    x4[..., :3] = x.permute(0, 2, 3, 4, 1)
    wp = torch.zeros(cout, 1, 3, 4, 4, dtype=torch.bfloat16, device="cuda")
    wp[:, :, :, :3, :3] = w.permute(0, 2, 3, 4, 1)
    cp = (cout + 7) // 8 * 8
    taps = torch.zeros(dk, cp, device="cuda")
    taps[:, :cout] = wt.reshape(cout, dk).t()
    y = torch.full((B, To, Ho, Wo, cp), 5.0, dtype=torch.bfloat16, device="cuda")
    d = L.Conv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = x4.data_ptr(), wp.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * 4, To * Ho * Wo * cp, 4, cp
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, 4, To, Ho, Wo, cout
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = 1, 3, 3, 1, 2, 2, 0, 1, 1
    d.act, d.a_act, d.dtype = act, L.ACT_NONE, L.PV_BF16
    d.dwt_w, d.dwt_k = taps.data_ptr(), dk
    assert L.lib().pv_conv3d_dwt_supported(C.byref(d)) == 1
    call("pv_conv3d", d)
    assert rel_err(y[..., :cout].permute(0, 4, 1, 2, 3), want) <= 1e-2
    assert torch.all(y[..., cout:] == 0)
    # the fusion exists for the first-layer layout only: a wide input must be refused, not mis-computed
    d.cin, d.ldx = 8, 8
    assert L.lib().pv_conv3d_dwt_supported(C.byref(d)) == 0


@pytest.mark.parametrize("rows,Cc", [(1000, 96), (333, 192), (77, 384), (50, 768), (9, 1000)])
def test_layernorm_fp32_stream_to_bf16_operand(rows, Cc):
    """The bf16 MViT plan normalises its fp32 residual stream into the bf16 GEMM operand."""
    x = _rand((rows, Cc), 71, torch.float32, 2.0) + 0.5
    g, b = _rand((Cc,), 72, torch.float32), _rand((Cc,), 73, torch.float32)
    want = F.layer_norm(x, (Cc,), g, b, 1e-6)
    y = torch.zeros(rows, Cc, dtype=torch.bfloat16, device="cuda")
    d = L.RowsDesc()
    d.x, d.y, d.gamma, d.beta = x.data_ptr(), y.data_ptr(), g.data_ptr(), b.data_ptr()
    d.rows, d.C, d.ldx, d.ldy, d.eps, d.dtype, d.x_f32 = rows, Cc, Cc, Cc, 1e-6, L.PV_BF16, 1
    call("pv_layernorm", d)
    assert rel_err(y, want) <= 1e-2


@pytest.mark.parametrize("stride,act", [((1, 1, 1), L.ACT_SWISH), ((1, 2, 2), L.ACT_NONE), ((1, 1, 1), L.ACT_RELU)])
@pytest.mark.parametrize("B,T,H,W,Cc", [(2, 5, 20, 23, 54), (1, 16, 7, 7, 432), (2, 3, 30, 9, 40)])
def test_depthwise_3x3x3_plane_kernel_with_se_partial_sums(B, T, H, W, Cc, stride, act):
    """X3D conv_b (bf16): output and the squeeze-excitation partial sums against torch."""
    cp = (Cc + 7) // 8 * 8
    x = torch.zeros(B, T, H, W, cp, dtype=torch.bfloat16, device="cuda")
    x[..., :Cc] = _rand((B, T, H, W, Cc), 81, torch.bfloat16)
    w = _rand((Cc, 1, 3, 3, 3), 82, torch.float32, 0.3)
    scale, shift = _rand((Cc,), 83, torch.float32) * 0.2 + 1.0, _rand((Cc,), 84, torch.float32)
    pre = F.conv3d(x[..., :Cc].float().permute(0, 4, 1, 2, 3), w, None, stride=stride, padding=1, groups=Cc)
    pre = pre * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    want = pre * torch.sigmoid(pre) if act == L.ACT_SWISH else (F.relu(pre) if act == L.ACT_RELU else pre)
    To, Ho, Wo = pre.shape[2:]
    y = torch.full((B, To, Ho, Wo, cp), 3.0, dtype=torch.bfloat16, device="cuda")
    wp = torch.zeros(27, cp, device="cuda")
    wp[:, :Cc] = w.reshape(Cc, 27).t()
    d = L.DwConv3dDesc()
    d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), wp.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cp, To * Ho * Wo * cp, cp, cp
    d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = B, T, H, W, Cc, To, Ho, Wo
    d.kt = d.kh = d.kw = 3
    d.st, d.sh, d.sw = stride
    d.pt = d.ph = d.pw = 1
    d.w_mod, d.act, d.dtype, d.n_prefix = 0, act, L.PV_BF16, 0
    nblk = L.lib().pv_dwconv3d_psum_blocks(C.byref(d))
    assert nblk > 0
    psum = torch.full((B, nblk, cp), float("nan"), device="cuda")
    d.psum = psum.data_ptr()
    call("pv_dwconv3d", d)
    assert rel_err(y[..., :Cc].permute(0, 4, 1, 2, 3), want) <= 1e-2
    assert torch.all(y[..., Cc:] == 0)
    got_mean = psum.sum(1)[:, :Cc] / (To * Ho * Wo)
    assert rel_err(got_mean, pre.mean(dim=[2, 3, 4])) <= 1e-3   # sums are fp32, before the bf16 rounding


@pytest.mark.parametrize("B,S,K,N,act,y_f32,pad", [
    (32, 1, 560, 2048, L.ACT_RELU, 0, 0),     # 35 K-steps over 8 waves, wide output
    (32, 1, 2048, 400, L.ACT_NONE, 1, 0),     # X3D-M head.proj: fp32 logits, 13 channel tiles (the last one ragged)
    (16, 4, 2304, 400, L.ACT_NONE, 1, 0),     # SlowFast-R50 head.proj on a 2x2 map: 64 rows, two row tiles
    (8, 1, 768, 400, L.ACT_NONE, 1, 16),      # MViT-B head on the cls rows, output wider than cout
    (5, 1, 520, 50, L.ACT_SIGMOID, 0, 0),     # ragged rows, K % 16 == 8, cout % 8 != 0 (padding channels written as 0)
    (11, 3, 768, 96, L.ACT_SWISH, 0, 8),      # 33 rows: second row tile almost empty
    (50, 4, 512, 40, L.ACT_NONE, 1, 0),       # 200 rows: four 64-row tiles (the batch never decides the routing)
])
def test_pointwise_conv_on_a_handful_of_rows_head_kernel(B, S, K, N, act, y_f32, pad):
    """csrc/pv_headgemm.hip (K-parallel, operands straight from global memory into MFMA layout) against fp32 torch, and
    bit-comparable with the tiled kernels it replaces on these shapes (same products, different summation order)."""
    kp, n8 = (K + 7) // 8 * 8, (N + 7) // 8 * 8
    x = torch.zeros(B, S, kp, dtype=torch.bfloat16, device="cuda")
    x[..., :K] = _rand((B, S, K), 301, torch.bfloat16)
    w = torch.zeros(N, kp, dtype=torch.bfloat16, device="cuda")
    w[:, :K] = _rand((N, K), 302, torch.bfloat16, K ** -0.5)
    scale, shift = _rand((N,), 303, torch.float32) * 0.2 + 1.0, _rand((N,), 304, torch.float32)
    pre = torch.einsum("bsk,nk->bsn", x[..., :K].float(), w[:, :K].float()) * scale + shift
    want = {L.ACT_NONE: pre, L.ACT_RELU: F.relu(pre), L.ACT_SIGMOID: torch.sigmoid(pre), L.ACT_SWISH: pre * torch.sigmoid(pre)}[act]
    ldy = n8 + pad
    outs = []
    try:
        for head_rows in (1, 0):
            L.tune(head_rows=head_rows)
            y = torch.full((B, S, ldy), 7.0, dtype=torch.float32 if y_f32 else torch.bfloat16, device="cuda")
            d = L.Conv3dDesc()
            d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
            d.x_bs, d.y_bs, d.ldx, d.ldy = S * kp, S * ldy, kp, ldy
            d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, 1, 1, S, kp, 1, 1, S, N
            d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
            d.act, d.a_act, d.dtype, d.y_f32 = act, L.ACT_NONE, L.PV_BF16, y_f32
            call("pv_conv3d", d)
            outs.append(y)
            if head_rows:
                assert rel_err(y[..., :N], want) <= (1e-4 if y_f32 else 1e-2)
                assert torch.all(y[..., N:n8] == 0) and torch.all(y[..., n8:] == 7.0)     # padding channels 0, nothing beyond
    finally:
        L.tune(head_rows=1)
    assert rel_err(outs[0][..., :N], outs[1][..., :N]) <= (1e-5 if y_f32 else 8e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,H,W,Cc,k,stride,pad,mode", [
    (2, 4, 14, 14, 96, (3, 3, 3), (1, 2, 2), (1, 1, 1), L.POOL_MAX),     # MViT skip-path pool
    (2, 3, 17, 13, 64, (1, 3, 3), (1, 2, 2), (0, 1, 1), L.POOL_MAX),     # stem pool, ragged edges
    (1, 5, 9, 9, 40, (3, 3, 3), (2, 1, 1), (1, 1, 1), L.POOL_AVG),       # average, temporal stride, padded count
    (2, 4, 8, 8, 24, (2, 2, 2), (2, 2, 2), (0, 0, 0), L.POOL_MAX),       # a window the unrolled kernel does not take
])
def test_pool3d_windows(dtype, B, T, H, W, Cc, k, stride, pad, mode):
    """pv_pool3d (MaxPool3d / AvgPool3d of models/stem.py:98-104, layers/attention.py:677-679): the unrolled 3x3x3 / 1x3x3 kernel
    against torch and bit-identical to the runtime-loop kernel."""
    cp = (Cc + 7) // 8 * 8
    x = torch.zeros(B, T, H, W, cp, dtype=dtype, device="cuda")
    x[..., :Cc] = _rand((B, T, H, W, Cc), 501, dtype)
    xin = x[..., :Cc].float().permute(0, 4, 1, 2, 3)
    want = F.max_pool3d(xin, k, stride, pad) if mode == L.POOL_MAX else F.avg_pool3d(xin, k, stride, pad, count_include_pad=True)
    To, Ho, Wo = want.shape[2:]
    outs = []
    try:
        for win in (1, 0):
            L.tune(pool_window=win)
            y = torch.full((B, To, Ho, Wo, cp), 3.0, dtype=dtype, device="cuda")
            d = L.Pool3dDesc()
            d.x, d.y, d.x_bs, d.y_bs, d.ldx, d.ldy = x.data_ptr(), y.data_ptr(), T * H * W * cp, To * Ho * Wo * cp, cp, cp
            d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = B, T, H, W, Cc, To, Ho, Wo
            d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *stride, *pad)
            d.mode, d.n_prefix, d.dtype = mode, 0, pv_dtype(x)
            call("pv_pool3d", d)
            outs.append(y)
    finally:
        L.tune(pool_window=1)
    assert rel_err(outs[0][..., :Cc].permute(0, 4, 1, 2, 3), want) <= (1e-6 if dtype == torch.float32 else 4e-3)
    assert torch.all(outs[0][..., Cc:] == 0) and torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ projection shortcut as a second K operand
@pytest.mark.parametrize("B,T,H,W,cin,cout,cin2,stride,gate", [
    (2, 4, 12, 10, 54, 24, 24, (1, 2, 2), True),      # X3D res2 block 0: SE gate + swish on the first operand only
    (2, 3, 9, 7, 108, 48, 24, (1, 2, 2), False),      # res3 block 0: 4 + 1 k-steps (generic K loop)
    (1, 4, 8, 8, 64, 256, 64, (1, 1, 1), False),      # ResNet res2 block 0: unstrided projection, 128-column slabs
    (3, 2, 6, 6, 40, 24, 16, (2, 2, 2), True),        # temporal stride, ragged channel counts
])
def test_pointwise_conv_with_projection_shortcut_as_second_operand(B, T, H, W, cin, cout, cin2, stride, gate):
    """ResBlock.forward (models/resnet.py:1179-1189) with branch1 folded into conv_c:
    y = relu(s1*(W1.h') + s2*(W2.x2s) + shift), h' = swish(h*gate) for squeeze-excited blocks, x2s = the block
    input sampled at the shortcut's stride; the two products keep their own fp32 BatchNorm scales."""
    st = stride
    T2, H2, W2 = (T - 1) * st[0] + 1, (H - 1) * st[1] + 1 + (st[1] > 1), (W - 1) * st[2] + 1
    assert ((T2 - 1) // st[0] + 1, (H2 - 1) // st[1] + 1, (W2 - 1) // st[2] + 1) == (T, H, W)
    cp1, cp2, cpo = (cin + 7) // 8 * 8, (cin2 + 7) // 8 * 8, (cout + 7) // 8 * 8
    h = torch.zeros(B, T, H, W, cp1, dtype=torch.bfloat16, device="cuda")
    h[..., :cin] = _rand((B, T, H, W, cin), 161, torch.bfloat16)
    x2 = torch.zeros(B, T2, H2, W2, cp2, dtype=torch.bfloat16, device="cuda")
    x2[..., :cin2] = _rand((B, T2, H2, W2, cin2), 162, torch.bfloat16)
    w1 = _rand((cout, cin), 163, torch.bfloat16, cin ** -0.5)
    w2 = _rand((cout, cin2), 164, torch.bfloat16, cin2 ** -0.5)
    shift = _rand((cout,), 165, torch.float32)
    s1, s2 = _rand((cout,), 166, torch.float32) * 0.2 + 1.0, _rand((cout,), 167, torch.float32) * 0.2 + 0.7
    g = (torch.rand(B, cp1, device="cuda") * 0.8 + 0.1) if gate else None
    hp = h[..., :cin].float()
    if gate:
        hp = hp * g[:, :cin].view(B, 1, 1, 1, cin)
        hp = (hp * torch.sigmoid(hp)).to(torch.bfloat16).float()
    x2s = x2[:, ::st[0], ::st[1], ::st[2], :cin2].float()
    want = F.relu((hp @ w1.float().t()) * s1 + (x2s @ w2.float().t()) * s2 + shift)
    k1, k2 = (cin + 31) // 32 * 32, (cin2 + 31) // 32 * 32
    wcat = torch.zeros(cout, k1 + k2, dtype=torch.bfloat16, device="cuda")
    wcat[:, :cin], wcat[:, k1:k1 + cin2] = w1, w2
    y = torch.full((B, T, H, W, cpo), 5.0, dtype=torch.bfloat16, device="cuda")
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
    assert rel_err(y[..., :cout], want) <= 1e-2
    assert torch.all(y[..., cout:] == 0)


# ------------------------------------------------------------------ squeeze-excitation gate
@pytest.mark.parametrize("B,Cc,cr,nblk", [
    (3, 54, 8, 56), (2, 108, 8, 14), (2, 216, 16, 4), (4, 432, 32, 2), (2, 40, 8, 1),
    (2, 600, 40, 3),     # beyond the register-resident variant: generic kernel
])
def test_se_gate_from_partial_sums(B, Cc, cr, nblk):
    """fvcore SqueezeExcitation as used at models/x3d.py:190-198: sigmoid(W2 relu(W1 mean + b1) + b2),
    the mean assembled from the depthwise kernel's per-tile partial sums."""
    cp = (Cc + 7) // 8 * 8
    psum = torch.zeros(B, nblk, cp, device="cuda")
    psum[..., :Cc] = _rand((B, nblk, Cc), 111, torch.float32, 3.0)
    w1, b1 = _rand((cr, Cc), 112, torch.float32, Cc ** -0.5), _rand((cr,), 113, torch.float32)
    w2, b2 = _rand((Cc, cr), 114, torch.float32, cr ** -0.5), _rand((Cc,), 115, torch.float32)
    count = 777.0
    mean = psum.sum(1)[:, :Cc] / count
    want = torch.sigmoid(F.relu(mean @ w1.t() + b1) @ w2.t() + b2)
    gate = torch.full((B, cp), 9.0, device="cuda")
    d = L.SeGateDesc()
    d.psum, d.gate, d.w1, d.b1, d.w2, d.b2 = psum.data_ptr(), gate.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    d.B, d.C, d.c_p, d.cr, d.nblk, d.inv_count = B, Cc, cp, cr, nblk, 1.0 / count
    call("pv_se_gate", d)
    assert rel_err(gate[:, :Cc], want) <= 1e-5
    assert torch.all(gate[:, Cc:] == 0)


# ------------------------------------------------------------------ conv_a fused into conv_b (pointwise producer)
@pytest.mark.parametrize("stride,act", [((1, 1, 1), L.ACT_SWISH), ((1, 2, 2), L.ACT_NONE)])
@pytest.mark.parametrize("B,T,H,W,Cin,Cc", [
    (2, 5, 20, 23, 24, 54),     # X3D res2 widths, ragged tiles, one k-step
    (1, 4, 14, 14, 96, 216),    # res4: three k-steps, seven channel slabs
    (1, 16, 7, 7, 192, 432),    # res5: narrow tiles (2 outputs per lane), six k-steps
    (2, 3, 30, 9, 48, 108),     # two k-steps
    (1, 3, 9, 40, 128, 40),     # four k-steps, output narrower than the input
])
def test_pointwise_conv_fused_into_depthwise_3x3x3(B, T, H, W, Cin, Cc, stride, act):
    """X3D conv_a+norm_a+ReLU -> conv_b+norm_b(+act) in one launch (csrc/pv_pwdw.hip): against torch,
    and bit-identical to the unfused pv_conv3d -> pv_dwconv3d pair (same bf16 rounding point)."""
    cp, cinp = (Cc + 7) // 8 * 8, (Cin + 7) // 8 * 8
    x = torch.zeros(B, T, H, W, cinp, dtype=torch.bfloat16, device="cuda")
    x[..., :Cin] = _rand((B, T, H, W, Cin), 91, torch.bfloat16)
    wa = _rand((Cc, Cin), 92, torch.bfloat16, Cin ** -0.5)
    sa, ha = _rand((Cc,), 93, torch.float32) * 0.2 + 1.0, _rand((Cc,), 94, torch.float32) * 0.5
    w = _rand((Cc, 1, 3, 3, 3), 95, torch.float32, 0.3)
    scale, shift = _rand((Cc,), 96, torch.float32) * 0.2 + 1.0, _rand((Cc,), 97, torch.float32)
    # reference: fp32 math on the bf16 inputs, conv_a output rounded to bf16 like the stored tensor
    h = torch.einsum("bthwc,oc->bthwo", x[..., :Cin].float(), wa.float()) * sa + ha
    h = F.relu(h).to(torch.bfloat16).float()
    pre = F.conv3d(h.permute(0, 4, 1, 2, 3), w, None, stride=stride, padding=1, groups=Cc)
    pre = pre * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    want = pre * torch.sigmoid(pre) if act == L.ACT_SWISH else pre
    To, Ho, Wo = pre.shape[2:]
    wp = torch.zeros(27, cp, device="cuda")
    wp[:, :Cc] = w.reshape(Cc, 27).t()

    def dw_desc(src, ld, y, psum):
        d = L.DwConv3dDesc()
        d.x, d.w, d.y, d.scale, d.shift = src.data_ptr(), wp.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
        d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * ld, To * Ho * Wo * cp, ld, cp
        d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = B, T, H, W, Cc, To, Ho, Wo
        d.kt = d.kh = d.kw = 3
        d.st, d.sh, d.sw = stride
        d.pt = d.ph = d.pw = 1
        d.w_mod, d.act, d.dtype, d.n_prefix = 0, act, L.PV_BF16, 0
        d.psum = psum.data_ptr()
        return d

    # fused
    y = torch.full((B, To, Ho, Wo, cp), 3.0, dtype=torch.bfloat16, device="cuda")
    wap = torch.zeros((Cc + 31) // 32 * 32, (Cin + 31) // 32 * 32, dtype=torch.bfloat16, device="cuda")
    wap[:Cc, :Cin] = wa
    d = dw_desc(x, cinp, y, torch.zeros(1, device="cuda"))
    d.pw_w, d.pw_scale, d.pw_shift, d.pw_cin, d.pw_act = wap.data_ptr(), sa.data_ptr(), ha.data_ptr(), Cin, L.ACT_RELU
    assert L.lib().pv_dwconv3d_pw_supported(C.byref(d)) == 1
    nblk = L.lib().pv_dwconv3d_psum_blocks(C.byref(d))
    psum = torch.full((B, nblk, cp), float("nan"), device="cuda")
    d.psum = psum.data_ptr()
    call("pv_dwconv3d", d)
    assert rel_err(y[..., :Cc].permute(0, 4, 1, 2, 3), want) <= 1e-2
    assert torch.all(y[..., Cc:] == 0)
    assert rel_err(psum.sum(1)[:, :Cc] / (To * Ho * Wo), pre.mean(dim=[2, 3, 4])) <= 2e-3

    # unfused pair through the same library
    hbuf = torch.zeros(B, T, H, W, cp, dtype=torch.bfloat16, device="cuda")
    wa8 = torch.zeros(Cc, cinp, dtype=torch.bfloat16, device="cuda")
    wa8[:, :Cin] = wa
    c = L.Conv3dDesc()
    c.x, c.w, c.y, c.scale, c.shift = x.data_ptr(), wa8.data_ptr(), hbuf.data_ptr(), sa.data_ptr(), ha.data_ptr()
    c.x_bs, c.y_bs, c.ldx, c.ldy = T * H * W * cinp, T * H * W * cp, cinp, cp
    c.B, c.Ti, c.Hi, c.Wi, c.cin, c.To, c.Ho, c.Wo, c.cout = B, T, H, W, cinp, T, H, W, Cc
    c.kt = c.kh = c.kw = c.st = c.sh = c.sw = 1
    c.act, c.a_act, c.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
    call("pv_conv3d", c)
    y2 = torch.full((B, To, Ho, Wo, cp), 5.0, dtype=torch.bfloat16, device="cuda")
    psum2 = torch.full((B, nblk, cp), float("nan"), device="cuda")
    call("pv_dwconv3d", dw_desc(hbuf, cp, y2, psum2))
    assert rel_err(y, y2) <= 2e-3   # same rounding points; MFMA accumulation order may differ in the last bit


# ------------------------------------------------------------------ fused q/k/v pooling + LayerNorm (one launch)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("heads,hd,thw,strides,cls", [
    (4, 96, (4, 14, 14), [(1, 1, 1), (1, 2, 2), (1, 2, 2)], 1),   # MViT-B block 4..13 (q unpooled there; all three here)
    (2, 96, (2, 16, 16), [(1, 2, 2), (1, 4, 4), (1, 4, 4)], 1),
    (1, 96, (4, 8, 8), [(1, 8, 8)], 1),
    (2, 64, (4, 6, 6), [(2, 2, 2), (1, 1, 1)], 0),
])
def test_fused_token_pooling_conv_layernorm(dtype, heads, hd, thw, strides, cls):
    B = 2
    T, H, W = thw
    Cw = heads * hd
    n = len(strides)
    d = L.TokenPoolDesc()
    keep, wants, outs = [], [], []
    for i, st in enumerate(strides):
        x = _rand((B, cls + T * H * W, Cw), 90 + i, dtype)
        w = _rand((hd, 1, 3, 3, 3), 95 + i, torch.float32, 0.3)
        g, bta = _rand((hd,), 100 + i, torch.float32) * 0.2 + 1.0, _rand((hd,), 105 + i, torch.float32) * 0.2
        grid = x[:, cls:].float().reshape(B, T, H, W, heads, hd).permute(0, 4, 5, 1, 2, 3).reshape(B * heads, hd, T, H, W)
        ref = F.conv3d(grid, w, None, stride=st, padding=1, groups=hd)
        To, Ho, Wo = ref.shape[2:]
        ref = ref.reshape(B, heads, hd, To * Ho * Wo).permute(0, 3, 1, 2)          # (B, L, heads, hd)
        if cls:
            ref = torch.cat([x[:, :1].float().reshape(B, 1, heads, hd), ref], 1)
        wants.append(F.layer_norm(ref, (hd,), g, bta, 1e-6).reshape(B, -1, Cw))
        y = torch.full((B, cls + To * Ho * Wo, Cw), 7.0, dtype=dtype, device="cuda")
        wp = w.reshape(hd, 27).t().contiguous()
        keep += [x, wp, g, bta]
        outs.append(y)
        d.x[i], d.y[i], d.w[i], d.gamma[i], d.beta[i] = x.data_ptr(), y.data_ptr(), wp.data_ptr(), g.data_ptr(), bta.data_ptr()
        d.x_bs[i], d.y_bs[i], d.ldx[i], d.ldy[i] = x.stride(0), y.stride(0), Cw, Cw
        d.st[i], d.sh[i], d.sw[i] = st
        d.To[i], d.Ho[i], d.Wo[i] = To, Ho, Wo
    d.n, d.B, d.Ti, d.Hi, d.Wi, d.heads, d.head_dim = n, B, T, H, W, heads, hd
    d.kt = d.kh = d.kw = 3
    d.n_prefix, d.eps, d.dtype = cls, 1e-6, pv_dtype(keep[0])
    call("pv_token_pool", d)
    for y, want in zip(outs, wants):
        assert rel_err(y, want) <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Ti,H,W,cin,cout,c_slow,kt,st", [
    (2, 32, 16, 16, 8, 16, 64, 7, 4),      # SlowFast-R50 site 1 (stem -> res2): 4 taps per K step
    (2, 32, 8, 8, 32, 64, 256, 7, 4),      # site 2
    (1, 32, 8, 8, 64, 128, 512, 7, 4),     # site 3
    (1, 32, 4, 4, 128, 256, 1024, 7, 4),   # site 4: the slab is split over channels
    (2, 16, 7, 9, 24, 40, 16, 5, 2),       # slowfast_r101's 5x1x1 kernel, alpha = 2, ragged spatial size and widths
    (1, 9, 5, 3, 16, 8, 8, 7, 4),          # fewer voxels than one wave tile, T not a multiple of alpha
])
def test_lateral_fusion_writes_the_slow_buffers_channel_slice(dtype, B, Ti, H, W, cin, cout, c_slow, kt, st):
    """pv_lateral_fuse vs F.conv3d + BatchNorm + ReLU + torch.cat (FuseFastToSlow.forward, models/slowfast.py:720-729)."""
    pt = kt // 2
    To = (Ti + 2 * pt - kt) // st + 1
    cin_p, cw = (cin + 7) // 8 * 8, c_slow + (cout + 7) // 8 * 8
    g = torch.Generator().manual_seed(11)
    xf = torch.zeros(B, Ti, H, W, cin_p)
    xf[..., :cin] = torch.randn(B, Ti, H, W, cin, generator=g)
    xf = xf.to(dtype).cuda()
    w = (torch.randn(cout, cin, kt, 1, 1, generator=g) * (1.5 / (cin * kt)) ** 0.5).to(dtype)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.rand(cout, generator=g) - 0.5
    slow = torch.randn(B, To, H, W, c_slow, generator=g).to(dtype)
    wide = torch.full((B, To, H, W, cw), 3.0, dtype=dtype)
    wide[..., :c_slow] = slow
    wide = wide.cuda()
    wp = torch.zeros(cout, kt, cin_p, dtype=dtype)
    wp[:, :, :cin] = w.reshape(cout, cin, kt).permute(0, 2, 1)
    wp, sc, sh = wp.cuda(), scale.cuda(), shift.cuda()
    d = L.LateralDesc()
    d.x, d.w, d.y = xf.data_ptr(), wp.data_ptr(), wide.data_ptr() + c_slow * wide.element_size()
    d.scale, d.shift = sc.data_ptr(), sh.data_ptr()
    d.x_bs, d.y_bs, d.ldx, d.ldy = xf.stride(0), wide.stride(0), cin_p, cw
    d.B, d.Ti, d.H, d.W, d.cin, d.To, d.cout = B, Ti, H, W, cin_p, To, cout
    d.kt, d.st, d.pt, d.act, d.dtype = kt, st, pt, L.ACT_RELU, pv_dtype(xf)
    call("pv_lateral_fuse", d)
    ref = F.conv3d(xf[..., :cin].float().cpu().permute(0, 4, 1, 2, 3), w.float(), stride=(st, 1, 1), padding=(pt, 0, 0))
    ref = F.relu(ref * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)).permute(0, 2, 3, 4, 1)
    got = wide.float().cpu()
    assert torch.equal(got[..., :c_slow], slow.float())                       # the slow pathway's slice is untouched
    assert rel_err(got[..., c_slow:c_slow + cout], ref) <= TOL[dtype]
    assert torch.all(got[..., c_slow + cout:] == 0)                           # padding channels of the slice are zeros


# ------------------------------------------------------------------ large-tile GEMM (256-voxel tiles, 4-stage LDS ring)
def _dense_gemm_case(ct, B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine, knob="gemm8", with_shift=True):
    """pv_conv3d forced onto one of the four dense GEMM kernels vs torch on the same bf16-rounded data: knob "gemm8" (ct = 2 | 4: the
    ring kernel's tile), "gemm9" / "gemm9h" (the eight-phase kernels) or "gemm" (the 128 x 128 kernel: conv_route = 2, the others
    off).  with_shift = False: no shift table.  The knobs are put back to the library's defaults (conv_route 0, gemm8 / gemm9 / gemm9h 1),
    as every test here does: the binding has no getter."""
    dtype = torch.bfloat16
    pad = tuple(kk // 2 for kk in k)
    g = torch.Generator().manual_seed(7 * cin + cout)
    x = torch.randn(B, T, H, W, cin, generator=g).to(dtype).cuda()
    w = (torch.randn((cout, cin) + k, generator=g) * (cin * k[0] * k[1] * k[2]) ** -0.5).to(dtype).cuda()
    shift = torch.randn(cout, generator=g).cuda()
    scale = (torch.rand(cout, generator=g) + 0.5).cuda() if affine else None
    if k == (1, 1, 1) and stride == (1, 1, 1):
        # the same sums as one fp32 matmul on the host (torch's own GPU conv spends up to a minute searching for an algorithm on a
        # 1 x 1 x 70 000 grid: 172 s of the suite in round 5)
        want = (x.float().cpu().reshape(-1, cin) @ w.float().cpu().reshape(cout, cin).t()).reshape(B, T, H, W, cout).permute(0, 4, 1, 2, 3).cuda()
    else:
        want = F.conv3d(x.float().permute(0, 4, 1, 2, 3), w.float(), stride=stride, padding=pad)
    if affine:
        want = want * scale.view(1, -1, 1, 1, 1)
    if with_shift:
        want = want + shift.view(1, -1, 1, 1, 1)
    To, Ho, Wo = want.shape[2:]
    cp = (cout + 7) // 8 * 8
    r = None
    if res:
        r = torch.randn(B, To, Ho, Wo, cp, generator=g).to(torch.float32 if y_f32 else dtype).cuda()
        want = want + r[..., :cout].float().permute(0, 4, 1, 2, 3)
    want = {L.ACT_NONE: lambda t: t, L.ACT_RELU: F.relu, L.ACT_GELU: F.gelu, L.ACT_SWISH: F.silu, L.ACT_SIGMOID: torch.sigmoid}[act](want)
    y = torch.full((B, To, Ho, Wo, cp), 5.0, dtype=torch.float32 if y_f32 else dtype, device="cuda")
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    d = L.Conv3dDesc()
    d.x, d.w, d.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
    d.shift = shift.data_ptr() if with_shift else None
    d.scale = scale.data_ptr() if affine else None
    d.residual = r.data_ptr() if res else None
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = T * H * W * cin, To * Ho * Wo * cp, To * Ho * Wo * cp, cin, cp, cp
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin, To, Ho, Wo, cout
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *stride, *pad)
    d.act, d.a_act, d.dtype, d.y_f32, d.r_f32 = act, L.ACT_NONE, L.PV_BF16, int(y_f32), int(y_f32 and res)
    if knob == "gemm":
        L.tune(conv_route=2, gemm8=0, gemm9=0)
    else:
        L.tune(**{knob: ct})
    if knob == "gemm8":                  # pv_conv3d asks the eight-phase kernels first: keep them away from the ring kernel's cases
        L.tune(gemm9=0)
    try:
        call("pv_conv3d", d)
        routed = _routed_kernel(L.OP_CONV3D, d)
        got1 = y.clone()
        call("pv_conv3d", d)                       # a second launch gives the same bits
    finally:
        if knob == "gemm":
            L.tune(conv_route=0, gemm8=1)
        else:
            L.tune(**{knob: 1})
        L.tune(gemm9=1)
    if knob == "gemm":
        assert routed == "gemm_glds_kernel", routed
    elif knob in ("gemm9", "gemm9h"):
        assert routed == {"gemm9": "gemm_quad_kernel", "gemm9h": "gemm_quad_half_kernel"}[knob], routed
    elif cin * k[0] * k[1] * k[2] >= 192 and (k == (1, 1, 1) or cin >= 64):
        # the ring kernel takes every forced case pv_conv3d offers it (pointwise, or >= 64 input channels) with at least three
        # 64-deep stages (these cases used to pass on the eight-phase kernels without reaching it)
        assert routed == "gemm8_kernel", routed
    assert torch.equal(got1, y)
    assert rel_err(y[..., :cout].permute(0, 4, 1, 2, 3), want) <= 1e-2
    if cp > cout:
        assert torch.all(y[..., cout:] == 0)       # padding channels are written as zeros


@pytest.mark.parametrize("ct", [2, 4])
@pytest.mark.parametrize("B,T,H,W,cin,cout,k,stride,act,res,y_f32,affine", [
    (1, 1, 1, 1000, 136, 200, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, False, True),     # ragged M, N and K tails
    (8, 1, 1, 785, 768, 768, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, True, False),      # MViT proj: fp32 stream in / out
    (2, 1, 1, 3137, 384, 1536, (1, 1, 1), (1, 1, 1), L.ACT_GELU, False, False, False),  # MViT fc1
    (1, 1, 1, 70000, 96, 120, (1, 1, 1), (1, 1, 1), L.ACT_NONE, False, False, False),   # > 256 tiles: several tiles per
                                                                                         # workgroup, shortest K (3 stages)
    (2, 8, 10, 10, 64, 96, (3, 1, 1), (1, 1, 1), L.ACT_RELU, False, False, True),       # SlowFast conv_a (3,1,1)
    (2, 4, 17, 13, 32, 136, (1, 3, 3), (1, 2, 2), L.ACT_RELU, True, False, True),       # conv_b (1,3,3), stride 2, odd grid
    (1, 32, 6, 6, 128, 256, (7, 1, 1), (4, 1, 1), L.ACT_RELU, False, False, True),      # lateral-shaped (7,1,1) / stride 4
])
def test_large_tile_gemm_kernel(ct, B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine):
    _dense_gemm_case(ct, B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine)


# ------------------------------------------------------------------ temporal-tap rotation / uniform-tap staging of the 128 x 128 GEMM
@pytest.mark.parametrize("B,T,H,W,cin,cout", [
    (2, 8, 16, 16, 64, 96),      # Ho*Wo % 128 == 0, cin % 64 == 0: rotation AND the uniform-tap fast path
    (2, 8, 16, 16, 128, 256),
    (2, 6, 16, 8, 72, 80),       # cin % 64 != 0: rotation without the fast path (per-chunk tap decoding)
])
def test_temporal_conv_tap_rotation_and_uniform_tap_staging(B, T, H, W, cin, cout):
    """(3,1,1) convs, pt = 1, st = 1, whole tiles inside one frame: the rotated tap order (pv_gemm.hip geom_of) and the
    wave-uniform tap staging are on by default -- against torch, and bit-for-bit against the same kernel with them switched off
    except for the summation order of the three taps (no kernel-level case reached the rotated path)."""
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(B, T, H, W, cin, generator=g).to(dtype).cuda()
    w = (torch.randn(cout, cin, 3, 1, 1, generator=g) * (3 * cin) ** -0.5).to(dtype).cuda()
    shift = torch.randn(cout, generator=g).cuda()
    want = F.relu(F.conv3d(x.float().permute(0, 4, 1, 2, 3), w.float(), padding=(1, 0, 0)) + shift.view(1, -1, 1, 1, 1))
    cp = (cout + 7) // 8 * 8
    wp = w.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()
    outs = {}
    for knobs in ({"gemm_tap_rot": 1, "gemm_tmode": 1}, {"gemm_tap_rot": 0, "gemm_tmode": 1}, {"gemm_tap_rot": 1, "gemm_tmode": 0},
                  {"gemm_tap_rot": 0, "gemm_tmode": 0}):
        y = torch.full((B, T, H, W, cp), 5.0, dtype=dtype, device="cuda")
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.shift = x.data_ptr(), wp.data_ptr(), y.data_ptr(), shift.data_ptr()
        d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin, T * H * W * cp, cin, cp
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin, T, H, W, cout
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = 3, 1, 1, 1, 1, 1, 1, 0, 0
        d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
        L.tune(conv_route=2, gemm8=0, gemm9=0, **knobs)
        try:
            call("pv_conv3d", d)
            assert _routed_kernel(L.OP_CONV3D, d) == "gemm_glds_kernel"
        finally:
            L.tune(conv_route=0, gemm8=1, gemm9=1, gemm_tap_rot=1, gemm_tmode=1)
        outs[tuple(sorted(knobs.items()))] = y
        assert rel_err(y[..., :cout].permute(0, 4, 1, 2, 3), want) <= 1e-2
    ys = list(outs.values())
    for other in ys[1:]:       # the same three products summed in another order: agreement to bf16 rounding of the output
        assert rel_err(other.float(), ys[0].float()) <= 8e-3
    k = lambda rot, tm: (("gemm_tap_rot", rot), ("gemm_tmode", tm))
    assert torch.equal(outs[k(0, 1)], outs[k(0, 0)])   # the fast path changes addresses, not arithmetic (without the temporal
    # fast path the general uniform-tap staging takes over where cin % 64 == 0, and that one does not rotate: (1, 0) == (0, 0))


# ------------------------------------------------------------------ 256 x 256 tiles, eight-phase main loop (pv_gemm9.hip, round 5)
@pytest.mark.parametrize("B,T,H,W,cin,cout,k,stride,act,res,y_f32,affine", [
    (1, 1, 1, 1000, 256, 200, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, False, True),     # ragged M and N tails, 4 K tiles
    (1, 1, 1, 100, 512, 72, (1, 1, 1), (1, 1, 1), L.ACT_NONE, False, False, False),     # less than one tile in M and N
    (8, 1, 1, 785, 768, 768, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, True, False),      # MViT proj: fp32 stream in / out
    (2, 1, 1, 3137, 384, 1536, (1, 1, 1), (1, 1, 1), L.ACT_GELU, False, False, False),  # MViT fc1
    (1, 1, 1, 70000, 256, 520, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, False, True),    # 822 tiles: several per workgroup (the
                                                                                         # DMA stream crosses tiles behind stores)
    (1, 1, 1, 40000, 256, 300, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, True, True),     # the same with fp32 stores (32 per tile)
    (2, 8, 10, 10, 128, 96, (3, 1, 1), (1, 1, 1), L.ACT_RELU, False, False, True),      # SlowFast conv_a (3,1,1): temporal padding
    (16, 8, 16, 16, 256, 256, (3, 1, 1), (1, 1, 1), L.ACT_RELU, False, False, True),    # ... at res4's grid, 128 tiles
    (2, 4, 17, 13, 128, 136, (1, 3, 3), (1, 2, 2), L.ACT_RELU, True, False, True),      # conv_b (1,3,3), stride 2, odd grid
    (3, 4, 16, 16, 128, 256, (1, 3, 3), (1, 1, 1), L.ACT_RELU, False, False, True),     # conv_b (1,3,3): spatial padding
    (2, 3, 9, 11, 128, 264, (3, 3, 3), (1, 1, 1), L.ACT_NONE, False, False, False),     # all three axes padded, 27 taps
    (1, 32, 6, 6, 128, 256, (7, 1, 1), (4, 1, 1), L.ACT_RELU, False, False, True),      # lateral-shaped (7,1,1) / stride 4
    (2, 4, 16, 16, 256, 512, (1, 1, 1), (1, 2, 2), L.ACT_NONE, False, False, True),     # projection shortcut: strided 1x1x1
])
def test_quad_phase_gemm_kernel(B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine):
    _dense_gemm_case(2, B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine, knob="gemm9")


# ------------------------------------------------------------------ the same loop on 128 x 256 tiles, three LDS buffers (pv_gemm9h.hip)
@pytest.mark.parametrize("B,T,H,W,cin,cout,k,stride,act,res,y_f32,affine", [
    (1, 1, 1, 1000, 384, 200, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, False, True),     # ragged M and N tails, 2 K-tile triples
    (1, 1, 1, 100, 576, 72, (1, 1, 1), (1, 1, 1), L.ACT_NONE, False, False, False),     # less than one tile in M and N
    (8, 1, 1, 785, 768, 768, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, True, False),      # MViT proj: fp32 stream in / out
    (2, 1, 1, 3137, 384, 1536, (1, 1, 1), (1, 1, 1), L.ACT_GELU, False, False, False),  # MViT fc1
    (1, 1, 1, 70000, 384, 520, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, False, True),    # 1641 tiles: several per workgroup (the
                                                                                         # DMA stream crosses tiles behind stores)
    (1, 1, 1, 40000, 384, 300, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, True, True),     # the same with fp32 stores (16 per tile)
    (2, 8, 10, 10, 128, 96, (3, 1, 1), (1, 1, 1), L.ACT_RELU, False, False, True),      # SlowFast conv_a (3,1,1): temporal padding
    (16, 8, 16, 16, 256, 256, (3, 1, 1), (1, 1, 1), L.ACT_RELU, False, False, True),    # ... at res4's grid, 256 tiles
    (2, 4, 17, 13, 64, 136, (1, 3, 3), (1, 2, 2), L.ACT_RELU, True, False, True),       # conv_b (1,3,3), stride 2, odd grid
    (3, 4, 16, 16, 128, 256, (1, 3, 3), (1, 1, 1), L.ACT_RELU, False, False, True),     # conv_b (1,3,3): spatial padding
    (16, 8, 8, 8, 512, 512, (1, 3, 3), (1, 1, 1), L.ACT_RELU, False, False, True),      # res5 conv_b: 72 K tiles, 128 tiles
    (2, 3, 9, 11, 64, 264, (3, 3, 3), (1, 1, 1), L.ACT_NONE, False, False, False),      # all three axes padded, 27 taps
    (1, 32, 6, 6, 192, 256, (7, 1, 1), (4, 1, 1), L.ACT_RELU, False, False, True),      # lateral-shaped (7,1,1) / stride 4
    (2, 4, 16, 16, 384, 512, (1, 1, 1), (1, 2, 2), L.ACT_NONE, False, False, True),     # projection shortcut: strided 1x1x1
])
def test_quad_phase_gemm_kernel_on_half_height_tiles(B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine):
    _dense_gemm_case(2, B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine, knob="gemm9h")


@pytest.mark.parametrize("B,T,H,W,cin,cout,k,stride,act,res,y_f32,affine", [
    (1, 1, 1, 1000, 384, 100, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, False, True),     # ragged M and N tails
    (1, 1, 1, 100, 576, 72, (1, 1, 1), (1, 1, 1), L.ACT_NONE, False, False, False),     # less than one tile in M and N
    (8, 1, 1, 785, 768, 384, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, True, False),      # fp32 stream in / out, three channel tiles
    (1, 1, 1, 70000, 384, 260, (1, 1, 1), (1, 1, 1), L.ACT_NONE, True, False, True),    # 822 tiles: several per workgroup
    (1, 1, 1, 40000, 384, 128, (1, 1, 1), (1, 1, 1), L.ACT_RELU, True, True, True),     # the same with fp32 stores
    (2, 8, 10, 10, 128, 96, (3, 1, 1), (1, 1, 1), L.ACT_RELU, False, False, True),      # (3,1,1): temporal padding
    (16, 8, 32, 32, 128, 128, (1, 3, 3), (1, 1, 1), L.ACT_RELU, False, False, True),    # SlowFast res3 conv_b at full size: 512 tiles
    (2, 4, 17, 13, 64, 136, (1, 3, 3), (1, 2, 2), L.ACT_RELU, True, False, True),       # stride 2, odd grid, two channel tiles
    (2, 3, 9, 11, 64, 120, (3, 3, 3), (1, 1, 1), L.ACT_NONE, False, False, False),      # all three axes padded, 27 taps
    (1, 32, 6, 6, 192, 128, (7, 1, 1), (4, 1, 1), L.ACT_RELU, False, False, True),      # lateral-shaped (7,1,1) / stride 4
    (2, 4, 16, 16, 384, 256, (1, 1, 1), (1, 2, 2), L.ACT_NONE, False, False, True),     # projection shortcut: strided 1x1x1
])
def test_quad_phase_gemm_kernel_on_transposed_half_tiles(B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine):
    """pv_gemm9h.hip with the 256 (voxels) x 128 (channels) tile: the voxel rows are the split operand."""
    L.tune(gemm9h_tr=1)
    try:
        _dense_gemm_case(2, B, T, H, W, cin, cout, k, stride, act, res, y_f32, affine, knob="gemm9h")
    finally:
        L.tune(gemm9h_tr=-1)




# the epilogue branches no other kernel-level case reaches, on each of the four dense GEMM kernels: pointwise, M = 100 (less than one
# tile, an M tail), K = 384 (the smallest all four accept), 70 channels (a ragged last channel tile, two padding channels)
@pytest.mark.parametrize("knob", ["gemm", "gemm8", "gemm9", "gemm9h"])
@pytest.mark.parametrize("act,res_f32,affine,with_shift", [
    (L.ACT_SWISH, False, True, False),      # swish, scale without shift, bf16 residual
    (L.ACT_SIGMOID, True, False, True),     # sigmoid, shift without scale, fp32 residual and output
])
def test_dense_gemm_epilogue_swish_sigmoid_scale_only_shift_only(knob, act, res_f32, affine, with_shift):
    _dense_gemm_case(2, 1, 1, 1, 100, 384, 70, (1, 1, 1), (1, 1, 1), act, True, res_f32, affine, knob=knob, with_shift=with_shift)


# temporal-tap rotation of the eight-phase kernels (whole tiles inside one output frame, temporal stride 1): the tile of output
# frame t starts its reduction at tap (pt - t) mod kt and wraps through weight column 0
@pytest.mark.parametrize("knob,tr,B,T,H,W,cin,cout,k,stride", [
    ("gemm9", -1, 16, 8, 16, 16, 256, 256, (3, 1, 1), (1, 1, 1)),     # SlowFast res4 conv_a: a frame = one 256-voxel tile
    ("gemm9", -1, 2, 5, 16, 16, 384, 256, (5, 1, 1), (1, 1, 1)),      # five taps, pt = 2: every rotation 0..4 occurs
    ("gemm9", -1, 2, 4, 16, 16, 128, 256, (3, 3, 3), (1, 1, 1)),      # 27 taps: the rotation moves only the temporal index
    ("gemm9", -1, 2, 8, 10, 10, 128, 96, (3, 1, 1), (1, 1, 1)),       # tiles straddle frames: not rotated (same stream code)
    ("gemm9h", 0, 16, 8, 16, 16, 256, 256, (3, 1, 1), (1, 1, 1)),     # two 128-voxel tiles per frame
    ("gemm9h", 0, 2, 5, 16, 16, 384, 256, (5, 1, 1), (1, 1, 1)),
    ("gemm9h", 0, 4, 6, 16, 8, 128, 96, (3, 1, 1), (1, 1, 1)),        # a frame = exactly one 128-voxel tile
    ("gemm9h", 0, 2, 4, 16, 16, 128, 256, (3, 3, 3), (1, 1, 1)),
    ("gemm9h", 0, 2, 8, 10, 10, 128, 96, (3, 1, 1), (1, 1, 1)),
    ("gemm9h", 1, 16, 8, 16, 16, 256, 128, (3, 1, 1), (1, 1, 1)),     # transposed tile: a frame = one 256-voxel tile
    ("gemm9h", 1, 2, 5, 16, 16, 384, 256, (5, 1, 1), (1, 1, 1)),
    ("gemm9h", 1, 2, 4, 16, 16, 128, 120, (3, 3, 3), (1, 1, 1)),
])
def test_eight_phase_kernels_temporal_tap_rotation(knob, tr, B, T, H, W, cin, cout, k, stride):
    L.tune(gemm9h_tr=tr)
    try:
        _dense_gemm_case(2, B, T, H, W, cin, cout, k, stride, L.ACT_RELU, False, False, True, knob=knob)
        L.tune(gemm9_tap_rot=0)            # ... and the same stream code without the rotation
        _dense_gemm_case(2, B, T, H, W, cin, cout, k, stride, L.ACT_RELU, False, False, True, knob=knob)
    finally:
        L.tune(gemm9h_tr=-1, gemm9_tap_rot=1)


@pytest.mark.parametrize("B,T,H,W,cin,cout,k,stride", [
    (2, 8, 16, 16, 8, 8, (1, 3, 3), (1, 1, 1)),      # SlowFast fast pathway res2 conv_b: 16 bytes per voxel
    (2, 8, 16, 16, 32, 8, (3, 1, 1), (1, 1, 1)),     # ... conv_a (3,1,1)
    (1, 6, 17, 13, 16, 16, (1, 3, 3), (1, 2, 2)),    # stride 2, odd grid
    (2, 5, 9, 7, 64, 32, (3, 1, 1), (1, 1, 1)),      # res4 fast conv_a
    (1, 4, 10, 12, 24, 40, (3, 3, 3), (2, 1, 2)),    # every tap direction at once, temporal stride, ragged widths
    (1, 3, 6, 6, 128, 32, (3, 1, 1), (1, 1, 1)),     # wide input, narrow output
    (2, 3, 12, 12, 64, 64, (1, 3, 3), (1, 1, 1)),    # SlowFast / ResNet res2 conv_b: taken BEFORE the 128-wide GEMM
])
def test_narrow_dense_conv_on_the_tap_streaming_kernel(B, T, H, W, cin, cout, k, stride):
    """pv_conv3d for narrow dense convolutions (csrc/pv_lateral.hip, pv_tapstream_try) vs torch, and the same op with
    the kernel switched off (generic implicit GEMM) to the last bit of bf16."""
    dtype = torch.bfloat16
    pad = tuple(kk // 2 for kk in k)
    g = torch.Generator().manual_seed(3 * cin + cout)
    cin_p = (cin + 7) // 8 * 8
    x = torch.zeros(B, T, H, W, cin_p)
    x[..., :cin] = torch.randn(B, T, H, W, cin, generator=g)
    x = x.to(dtype).cuda()
    w = (torch.randn((cout, cin) + k, generator=g) * (cin * k[0] * k[1] * k[2]) ** -0.5).to(dtype)
    scale, shift = (torch.rand(cout, generator=g) + 0.5).cuda(), (torch.rand(cout, generator=g) - 0.5).cuda()
    want = F.conv3d(x[..., :cin].float().cpu().permute(0, 4, 1, 2, 3), w.float(), stride=stride, padding=pad)
    want = F.relu(want * scale.cpu().view(1, -1, 1, 1, 1) + shift.cpu().view(1, -1, 1, 1, 1))
    To, Ho, Wo = want.shape[2:]
    cp = (cout + 7) // 8 * 8
    wp = torch.zeros(cout, k[0] * k[1] * k[2], cin_p, dtype=dtype)
    wp[:, :, :cin] = w.permute(0, 2, 3, 4, 1).reshape(cout, -1, cin)
    wp = wp.cuda()

    def run(tap):
        y = torch.full((B, To, Ho, Wo, cp), 5.0, dtype=dtype, device="cuda")
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), wp.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr()
        d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin_p, To * Ho * Wo * cp, cin_p, cp
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin_p, To, Ho, Wo, cout
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *stride, *pad)
        d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
        L.tune(tapstream=tap, tapstream_first=tap)
        try:
            call("pv_conv3d", d)
        finally:
            L.tune(tapstream=1, tapstream_first=1)
        return y

    y1, y0 = run(1), run(0)
    assert rel_err(y1[..., :cout].permute(0, 4, 1, 2, 3), want) <= 1e-2
    assert torch.all(y1[..., cout:] == 0)
    assert rel_err(y1, y0) <= 4e-3      # the generic kernel: same products, other summation order


# ------------------------------------------------------------------ conv_b -> conv_c in one launch (pv_conv3d pw2_*, csrc/pv_lateral.hip)
@pytest.mark.parametrize("B,T,H,W,cin,cmid,cout2,k,stride,res,act_b", [
    (2, 4, 16, 16, 64, 64, 256, (1, 3, 3), (1, 1, 1), True, L.ACT_RELU),    # SlowFast / ResNet res2: 64 -> 64 -> 256 + identity
    (2, 8, 16, 16, 8, 8, 32, (1, 3, 3), (1, 1, 1), True, L.ACT_RELU),       # fast pathway res2: 8 -> 8 -> 32
    (1, 4, 13, 11, 16, 16, 64, (1, 3, 3), (1, 1, 1), False, L.ACT_RELU),    # ragged voxel tiles, no residual
    (2, 4, 12, 12, 32, 24, 72, (3, 1, 1), (1, 1, 1), True, L.ACT_RELU),     # inner / outer widths that are not multiples of 32
    (1, 6, 10, 10, 64, 64, 200, (1, 3, 3), (1, 2, 2), True, L.ACT_NONE),    # strided conv_b, no inner activation, ragged last 32 channels
    (1, 3, 9, 9, 16, 36, 20, (3, 3, 3), (1, 1, 1), False, L.ACT_RELU),      # every tap direction, 36 inner channels (8-padding inside a pair)
])
def test_conv_b_and_pointwise_conv_c_in_one_launch(B, T, H, W, cin, cmid, cout2, k, stride, res, act_b):
    """pv_conv3d with pw2_*: conv_b + BN + act -> (bf16) -> conv_c + BN + residual + ReLU, the inner tensor kept in registers as
    the second product's MFMA operand -- vs torch in fp32 with the inner tensor rounded to bf16 where the unfused pair stores
    it, and vs the unfused pair of pv_conv3d launches."""
    dtype = torch.bfloat16
    pad = tuple(kk // 2 for kk in k)
    g = torch.Generator().manual_seed(5 * cin + cmid + cout2)
    cin_p, cm_p, c2_p = (cin + 7) // 8 * 8, (cmid + 7) // 8 * 8, (cout2 + 7) // 8 * 8
    x = torch.zeros(B, T, H, W, cin_p)
    x[..., :cin] = torch.randn(B, T, H, W, cin, generator=g)
    x = x.to(dtype).cuda()
    taps = k[0] * k[1] * k[2]
    wb = (torch.randn((cmid, cin) + k, generator=g) * (cin * taps) ** -0.5).to(dtype)
    wc = (torch.randn(cout2, cmid, generator=g) * cmid ** -0.5).to(dtype)
    sb, hb = (torch.rand(cmid, generator=g) + 0.5).cuda(), (torch.rand(cmid, generator=g) - 0.5).cuda()
    sc, hc = (torch.rand(cout2, generator=g) + 0.5).cuda(), (torch.rand(cout2, generator=g) - 0.5).cuda()
    mid = F.conv3d(x[..., :cin].float().cpu().permute(0, 4, 1, 2, 3), wb.float(), stride=stride, padding=pad)
    mid = mid * sb.cpu().view(1, -1, 1, 1, 1) + hb.cpu().view(1, -1, 1, 1, 1)
    mid = (F.relu(mid) if act_b == L.ACT_RELU else mid).to(dtype).float()
    To, Ho, Wo = mid.shape[2:]
    want = torch.einsum("bcthw,oc->bothw", mid, wc.float()) * sc.cpu().view(1, -1, 1, 1, 1) + hc.cpu().view(1, -1, 1, 1, 1)
    r = None
    if res:
        r = torch.zeros(B, To, Ho, Wo, c2_p)
        r[..., :cout2] = torch.randn(B, To, Ho, Wo, cout2, generator=g)
        r = r.to(dtype).cuda()
        want = want + r[..., :cout2].float().cpu().permute(0, 4, 1, 2, 3)
    want = F.relu(want)
    wbp = torch.zeros(cmid, taps, cin_p, dtype=dtype)
    wbp[:, :, :cin] = wb.permute(0, 2, 3, 4, 1).reshape(cmid, -1, cin)
    wcp = torch.zeros(cout2, cm_p, dtype=dtype)
    wcp[:, :cmid] = wc
    wbp, wcp = wbp.cuda(), wcp.cuda()

    def conv_b_desc(y, ld, cout):
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.scale, d.shift = x.data_ptr(), wbp.data_ptr(), y.data_ptr(), sb.data_ptr(), hb.data_ptr()
        d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin_p, To * Ho * Wo * ld, cin_p, ld
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin_p, To, Ho, Wo, cout
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *stride, *pad)
        d.act, d.a_act, d.dtype = act_b, L.ACT_NONE, L.PV_BF16
        return d

    # one launch
    y1 = torch.full((B, To, Ho, Wo, c2_p), 5.0, dtype=dtype, device="cuda")
    d = conv_b_desc(y1, c2_p, cmid)
    d.pw2_w, d.pw2_scale, d.pw2_shift, d.pw2_cout, d.pw2_act = wcp.data_ptr(), sc.data_ptr(), hc.data_ptr(), cout2, L.ACT_RELU
    if res:
        d.residual, d.r_bs, d.ldr = r.data_ptr(), To * Ho * Wo * c2_p, c2_p
    assert L.lib().pv_conv3d_pw2_supported(C.byref(d)) == 1
    call("pv_conv3d", d)
    assert _routed_kernel(L.OP_CONV3D, d) == "tap_stream_kernel"
    first = y1.clone()
    call("pv_conv3d", d)
    assert torch.equal(first, y1)                       # a second launch gives the same bits
    # the unfused pair
    ym = torch.full((B, To, Ho, Wo, cm_p), 5.0, dtype=dtype, device="cuda")
    call("pv_conv3d", conv_b_desc(ym, cm_p, cmid))
    y0 = torch.full((B, To, Ho, Wo, c2_p), 5.0, dtype=dtype, device="cuda")
    e = L.Conv3dDesc()
    e.x, e.w, e.y, e.scale, e.shift = ym.data_ptr(), wcp.data_ptr(), y0.data_ptr(), sc.data_ptr(), hc.data_ptr()
    e.x_bs, e.y_bs, e.ldx, e.ldy = To * Ho * Wo * cm_p, To * Ho * Wo * c2_p, cm_p, c2_p
    e.B, e.Ti, e.Hi, e.Wi, e.cin, e.To, e.Ho, e.Wo, e.cout = B, To, Ho, Wo, cm_p, To, Ho, Wo, cout2
    e.kt = e.kh = e.kw = e.st = e.sh = e.sw = 1
    e.act, e.a_act, e.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
    if res:
        e.residual, e.r_bs, e.ldr = r.data_ptr(), To * Ho * Wo * c2_p, c2_p
    call("pv_conv3d", e)
    assert rel_err(y1[..., :cout2].permute(0, 4, 1, 2, 3), want) <= 1e-2
    assert torch.all(y1[..., cout2:] == 0)               # padding channels are written as zeros
    assert rel_err(y1, y0) <= 4e-3                       # same operands, same roundings; only the summation order differs


def test_pointwise_conv_behind_a_conv_is_declined_outside_the_streaming_kernels_range():
    """pv_conv3d_pw2_supported / pv_conv3d: more than 64 inner channels, a pointwise first conv, fp32 and a residual with other
    strides than the output are declined (the emitter then keeps the two launches); nothing falls back to another kernel."""
    def desc(cin=64, cmid=64, cout2=256, k=(1, 3, 3), dtype=L.PV_BF16):
        d = L.Conv3dDesc()
        B, T, H, W = 2, 4, 16, 16
        d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin, T * H * W * cout2, cin, cout2
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = B, T, H, W, cin, T, H, W, cmid
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, 1, 1, 1, *(kk // 2 for kk in k))
        d.dtype, d.pw2_cout = dtype, cout2
        return d
    sup = lambda d: L.lib().pv_conv3d_pw2_supported(C.byref(d))
    assert sup(desc()) == 1
    assert sup(desc(cmid=128)) == 0
    assert sup(desc(k=(1, 1, 1))) == 0
    assert sup(desc(dtype=L.PV_F32)) == 0
    assert sup(desc(cin=256, k=(3, 3, 3))) == 0          # K = 6912: not a streaming problem
    d = desc()
    d.residual, d.r_bs, d.ldr = 1, d.y_bs * 2, d.ldy      # (pointer value irrelevant for the geometry check)
    assert sup(d) == 0
    # and the launch itself declines what the check declines
    x = torch.zeros(2, 4, 16, 16, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(128, 9 * 64, dtype=torch.bfloat16, device="cuda")
    w2 = torch.zeros(256, 128, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(2, 4, 16, 16, 256, dtype=torch.bfloat16, device="cuda")
    d = desc(cmid=128)
    d.x, d.w, d.y, d.pw2_w = x.data_ptr(), w.data_ptr(), y.data_ptr(), w2.data_ptr()
    assert L.lib().pv_conv3d(C.byref(d), None) == L.PV_ERR_UNSUPPORTED


@pytest.mark.parametrize("M,Cin,H,Cout,ln,res", [
    (300, 96, 384, 192, False, True),       # MViT-B block 0 (width change: residual = proj(norm2(x)), own launch)
    (50, 96, 384, 96, True, False),         # 96 -> 96 with the LayerNorm in the kernel
    (1001, 192, 768, 192, True, False),     # block 1
    (257, 192, 768, 384, False, True),      # block 2
    (6274, 384, 1536, 384, True, False),    # blocks 3-12 (two clips of 3137 tokens)
    (130, 384, 1536, 384, False, False),    # bf16 operand, no residual
    (129, 384, 64, 384, True, False),       # two hidden blocks only
])
def test_fused_mlp_rows(M, Cin, H, Cout, ln, res):
    """pv_mlp_rows: norm2 -> fc1 -> GELU -> fc2 -> + residual (layers/attention.py:102-114,750-757) in one launch
    against fp32 torch on the same bf16-rounded weights (ragged row counts: the last 128-row tile is partial)."""
    from pytorchvideo_amd.accelerator.mi355x.emit_mvit import pack_mlp_weights
    g = torch.Generator().manual_seed(77)
    w1 = (torch.randn(H, Cin, generator=g) * Cin ** -0.5).bfloat16().float()
    w2 = (torch.randn(Cout, H, generator=g) * H ** -0.5).bfloat16().float()
    b1, b2 = torch.randn(H, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.3
    gamma, beta = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.2
    x32 = torch.randn(M, Cin, generator=g) * 2.0 + 3.0 * torch.randn(M, 1, generator=g)      # rows with a large mean
    r32 = torch.randn(M, Cout, generator=g)
    if ln:
        xn = F.layer_norm(x32, (Cin,), gamma, beta, 1e-6)
        want = x32 + b2 + F.linear(F.gelu(F.linear(xn, w1, b1)), w2)
        x_dev = x32.cuda()
    else:
        xb = x32.bfloat16()
        want = b2 + F.linear(F.gelu(F.linear(xb.float(), w1, b1)), w2) + (r32 if res else 0.0)
        x_dev = xb.cuda()
    img = pack_mlp_weights(w1, b1, w2).cuda()
    y = torch.full((M, Cout), 7.0, dtype=torch.float32, device="cuda")
    b2d, gd, bd, rd = b2.cuda(), gamma.cuda(), beta.cuda(), r32.cuda()
    d = L.MlpDesc()
    d.x, d.w12, d.y, d.b2 = x_dev.data_ptr(), img.data_ptr(), y.data_ptr(), b2d.data_ptr()
    d.residual = rd.data_ptr() if (res and not ln) else None
    d.ln_gamma, d.ln_beta, d.ln_eps = (gd.data_ptr(), bd.data_ptr(), 1e-6) if ln else (None, None, 0.0)
    d.M, d.C, d.H, d.Cout, d.ldx, d.ldr, d.ldy, d.act, d.dtype = M, Cin, H, Cout, Cin, Cout, Cout, L.ACT_GELU, L.PV_BF16
    assert L.lib().pv_mlp_rows_supported(C.byref(d)) == 1
    call("pv_mlp_rows", d)
    assert _routed_kernel(L.OP_MLP_ROWS, d) == "mlp_rows16_kernel"
    assert rel_err(y, want) <= 1e-2
    y2 = torch.zeros_like(y)
    d.y = y2.data_ptr()
    call("pv_mlp_rows", d)
    assert torch.equal(y, y2)                       # no atomics, fixed order: bitwise reproducible
    # round 4: norm1 of the NEXT block written from the rows the kernel still holds (d.yn): LayerNorm of the fp32 result as
    # a bf16 operand, against torch on the kernel's own y; y itself unchanged bit for bit; row stride wider than Cout
    ng, nb_ = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.2).cuda()
    ldn = Cout + 8
    yn = torch.full((M, ldn), 5.0, dtype=torch.bfloat16, device="cuda")
    y3 = torch.zeros_like(y)
    d.y, d.yn, d.nn_gamma, d.nn_beta, d.ldyn, d.nn_eps = y3.data_ptr(), yn.data_ptr(), ng.data_ptr(), nb_.data_ptr(), ldn, 1e-6
    call("pv_mlp_rows", d)
    assert torch.equal(y3, y)
    want_n = F.layer_norm(y3, (Cout,), ng, nb_, 1e-6)
    assert rel_err(yn[:, :Cout], want_n) <= 1e-2
    assert (yn[:, :Cout].float() - want_n).abs().max().item() <= 2.0 ** -7 * want_n.abs().max().item()   # one bf16 rounding
    assert torch.all(yn[:, Cout:] == 5.0)           # nothing written past the row
    d.ldyn = Cout - 8
    assert L.lib().pv_mlp_rows(C.byref(d), None) < 0      # inconsistent descriptor: rejected
    d.yn = None
    # unsupported widths are declined, inconsistent descriptors rejected
    d.C = 768
    assert L.lib().pv_mlp_rows_supported(C.byref(d)) == 0


@pytest.mark.parametrize("chans,B,T,H,W,act_b", [
    ((96, 216, 96), 2, 5, 14, 14, L.ACT_SWISH),     # X3D res4: 14 x 14 maps, seven 2-row tiles per clip
    ((96, 216, 96), 1, 3, 7, 9, L.ACT_SWISH),       # odd height (the last tile holds one row), narrower than a 14-column tile
    ((96, 216, 96), 3, 1, 2, 14, L.ACT_RELU),       # a single frame: both temporal neighbours are padding
    ((96, 216, 96), 1, 16, 13, 5, L.ACT_NONE),
    ((96, 216, 96), 1, 2, 5, 31, L.ACT_SWISH),      # three column tiles, the last one ragged (halo columns from the neighbours)
    ((48, 108, 48), 1, 4, 28, 28, L.ACT_SWISH),     # X3D res3: two column tiles, two 7-output row segments per stencil row
    ((48, 108, 48), 2, 3, 9, 17, L.ACT_RELU),
    ((24, 54, 24), 1, 3, 56, 56, L.ACT_SWISH),      # X3D res2: one channel per stencil lane, 24 output channels in a 32-channel tile
    ((24, 54, 24), 2, 2, 5, 30, L.ACT_NONE),
])
def test_fused_bottleneck_block(chans, B, T, H, W, act_b):
    """pv_bottleneck (round 6, csrc/pv_block.hip): conv_a + BN + ReLU -> depthwise 3x3x3 + BN + Swish -> conv_c + BN -> + x -> ReLU
    of an X3D res4 block (models/x3d.py:169-212, models/resnet.py:1345-1365, :1179-1189) in one launch, against fp32 torch on
    the same bf16-rounded operands -- plainly, and with the two intermediate tensors rounded to bf16 where the kernel rounds them."""
    import torch.nn as nn
    from pytorchvideo_amd.accelerator.mi355x.emit import pack_bottleneck_operands
    cin, Cc, cout = chans
    g = torch.Generator().manual_seed(100 * H + W)
    ca, cb, cc = nn.Conv3d(cin, Cc, 1, bias=False), nn.Conv3d(Cc, Cc, 3, padding=1, groups=Cc, bias=False), nn.Conv3d(Cc, cout, 1, bias=False)
    with torch.no_grad():
        ca.weight.copy_((torch.randn(Cc, cin, 1, 1, 1, generator=g) * cin ** -0.5).bfloat16().float())
        cb.weight.copy_(torch.randn(Cc, 1, 3, 3, 3, generator=g) * 27 ** -0.5)
        cc.weight.copy_((torch.randn(cout, Cc, 1, 1, 1, generator=g) * Cc ** -0.5).bfloat16().float())

    def bn(c):
        m = nn.BatchNorm3d(c).eval()
        with torch.no_grad():
            m.weight.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.copy_(torch.randn(c, generator=g) * 0.3)
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        return m

    na, nb, nc = bn(Cc), bn(Cc), bn(cout)
    fb = {L.ACT_SWISH: lambda t: t * torch.sigmoid(t), L.ACT_RELU: F.relu, L.ACT_NONE: lambda t: t}[act_b]
    x = torch.randn(B, T, H, W, cin, generator=g).bfloat16()
    xc = x.float().permute(0, 4, 1, 2, 3)
    q = lambda t: t.bfloat16().float()
    with torch.no_grad():
        want = F.relu(xc + nc(cc(fb(nb(cb(F.relu(na(ca(xc))))))))).permute(0, 2, 3, 4, 1)
        want_q = F.relu(xc + nc(cc(q(fb(nb(cb(q(F.relu(na(ca(xc))))))))))).permute(0, 2, 3, 4, 1)
    ops = {k: v.cuda() for k, v in pack_bottleneck_operands(ca, na, cb, nb, cc, nc).items()}
    xd = x.cuda()
    ldy = cout + 8
    y = torch.full((B, T, H, W, ldy), 5.0, dtype=torch.bfloat16, device="cuda")
    d = L.BottleneckDesc()
    d.x, d.y, d.residual = xd.data_ptr(), y.data_ptr(), xd.data_ptr()
    for k, v in ops.items():
        setattr(d, k, v.data_ptr())
    d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = T * H * W * cin, T * H * W * ldy, T * H * W * cin, cin, ldy, cin
    d.B, d.T, d.H, d.W, d.cin, d.C, d.cout = B, T, H, W, cin, Cc, cout
    d.act_a, d.act_b, d.act_out, d.dtype = L.ACT_RELU, act_b, L.ACT_RELU, L.PV_BF16
    assert L.lib().pv_bottleneck_supported(C.byref(d)) == 1
    call("pv_bottleneck", d)
    assert _routed_kernel(L.OP_BOTTLENECK, d) == "bottleneck_block_kernel"
    got = y[..., :cout]
    assert rel_err(got, want) <= 1e-2
    assert rel_err(got, want_q) <= 6e-3                 # one bf16 rounding of the result + fp32 summation order
    assert torch.all(y[..., cout:] == 5.0)              # nothing written beyond the block's channels
    y2 = torch.zeros_like(y)
    d.y = y2.data_ptr()
    call("pv_bottleneck", d)
    assert torch.equal(y2[..., :cout], got)             # no atomics: bit-reproducible
    d.C = 300                                           # a width the kernel is not instantiated for: declined, not mis-computed
    assert L.lib().pv_bottleneck_supported(C.byref(d)) == 0 and L.lib().pv_bottleneck(C.byref(d), None) < 0


@pytest.mark.parametrize("chans,B,T,H,W", [((96, 216), 2, 5, 14, 14), ((96, 216), 1, 3, 7, 9), ((96, 216), 2, 2, 13, 14),
                                           ((96, 216), 1, 2, 4, 20), ((48, 108), 1, 3, 28, 28), ((48, 108), 2, 2, 5, 9),
                                           ((24, 54), 1, 2, 56, 56), ((24, 54), 1, 3, 11, 33)])
def test_fused_bottleneck_conv_ab_with_squeeze_sums(chans, B, T, H, W):
    """pv_bottleneck in mode PV_BLOCK_AB (blocks with squeeze-excitation, models/x3d.py:169-207): conv_a + BN + ReLU -> depthwise
    3x3x3 + BN as bf16, and the per-block fp32 sums of the (unrounded) result whose total is the squeeze -- against fp32 torch."""
    import torch.nn as nn
    from pytorchvideo_amd.accelerator.mi355x.emit import pack_bottleneck_operands
    cin, Cc = chans
    g = torch.Generator().manual_seed(10 * H + W)
    ca, cb = nn.Conv3d(cin, Cc, 1, bias=False), nn.Conv3d(Cc, Cc, 3, padding=1, groups=Cc, bias=False)
    with torch.no_grad():
        ca.weight.copy_((torch.randn(Cc, cin, 1, 1, 1, generator=g) * cin ** -0.5).bfloat16().float())
        cb.weight.copy_(torch.randn(Cc, 1, 3, 3, 3, generator=g) * 27 ** -0.5)

    def bn(c):
        m = nn.BatchNorm3d(c).eval()
        with torch.no_grad():
            m.weight.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.copy_(torch.randn(c, generator=g) * 0.3)
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        return m

    na, nb = bn(Cc), bn(Cc)
    x = torch.randn(B, T, H, W, cin, generator=g).bfloat16()
    xc = x.float().permute(0, 4, 1, 2, 3)
    with torch.no_grad():
        want = nb(cb(F.relu(na(ca(xc))).bfloat16().float())).permute(0, 2, 3, 4, 1)       # the expanded tensor rounded where the kernel rounds it
    ops = {k: v.cuda() for k, v in pack_bottleneck_operands(ca, na, cb, nb, None, None).items()}
    xd = x.cuda()
    ldy = Cc + 8
    y = torch.full((B, T, H, W, ldy), 5.0, dtype=torch.bfloat16, device="cuda")
    d = L.BottleneckDesc()
    d.x, d.y, d.mode = xd.data_ptr(), y.data_ptr(), L.BLOCK_AB
    for k, v in ops.items():
        setattr(d, k, v.data_ptr())
    d.x_bs, d.y_bs, d.ldx, d.ldy = T * H * W * cin, T * H * W * ldy, cin, ldy
    d.B, d.T, d.H, d.W, d.cin, d.C, d.cout = B, T, H, W, cin, Cc, cin
    d.act_a, d.dtype = L.ACT_RELU, L.PV_BF16
    # by default this mode is routed for res4 only (on larger maps the plane-streaming kernel with the fused pointwise producer is
    # faster); the res2 / res3 instantiations exist and are tested under the knob
    assert L.lib().pv_bottleneck_supported(C.byref(d)) == (1 if Cc == 216 else 0)
    L.tune(block_stages_ab=0x1c)
    try:
        assert L.lib().pv_bottleneck_supported(C.byref(d)) == 1
        nblk = L.lib().pv_bottleneck_psum_blocks(C.byref(d))
        segs = 1 if Cc == 216 else 2
        assert nblk == (H + 1) // 2 * 2 * ((W + 13) // 14) * segs
        cp8 = (Cc + 7) // 8 * 8
        psum_p = torch.full((B, nblk, cp8), 7.0, device="cuda")               # [B][blocks][round_up(C, 8)]
        d.psum = psum_p.data_ptr()
        call("pv_bottleneck", d)
    finally:
        L.tune(block_stages_ab=0x10)
    got = y[..., :Cc]
    assert rel_err(got, want) <= 6e-3                                    # one bf16 rounding + fp32 summation order
    assert torch.all(y[..., Cc:cp8] == 0) and torch.all(y[..., cp8:] == 5.0)      # padding channels of the 8-channel chunk are zeros, nothing beyond
    assert torch.all(psum_p[..., Cc:] == 0)
    psum = psum_p[..., :Cc]
    sums = want.sum(dim=(1, 2, 3))                                         # [B, C]
    assert rel_err(psum.sum(dim=1), sums) <= 1e-4                          # fp32 sums of the unrounded values
    # per block: with one column tile and one segment, block 2 * tile + row holds output row 2 * tile + row of every frame
    if nblk == (H + 1) // 2 * 2:
        per_row = want.sum(dim=(1, 3))                                     # [B, H, C]
        assert rel_err(psum[:, :H], per_row) <= 1e-4
        if nblk > H:
            assert torch.all(psum[:, H:] == 0)


@pytest.mark.parametrize("M,Cin,N", [(300, 96, 288), (1001, 192, 576), (6274, 384, 1152), (129, 384, 96), (785 * 2, 768, 2304),
                                     (31, 96, 32)])
def test_layernorm_fused_into_the_qkv_linear(M, Cin, N):
    """pv_ln_linear_rows: norm1 -> q|k|v Linear (layers/attention.py:729-737,425-451) in one launch against fp32 torch
    on the same bf16-rounded weights; rows with a large mean (shifted one-pass statistics), ragged last tile, a last
    workgroup whose trailing waves hold no row at all."""
    from pytorchvideo_amd.accelerator.mi355x.emit_mvit import pack_ln_linear_weights
    g = torch.Generator().manual_seed(78)
    w = (torch.randn(N, Cin, generator=g) * Cin ** -0.5).bfloat16().float()
    b = torch.randn(N, generator=g) * 0.3
    gamma, beta = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.2
    x = torch.randn(M, Cin, generator=g) * 2.0 + 5.0 * torch.randn(M, 1, generator=g)
    want = F.linear(F.layer_norm(x, (Cin,), gamma, beta, 1e-6), w, b)
    img = pack_ln_linear_weights(w, b).cuda()
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    y = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
    d = L.LnLinearDesc()
    d.x, d.wb, d.y, d.ln_gamma, d.ln_beta = xd.data_ptr(), img.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr()
    d.M, d.C, d.N, d.ldx, d.ldy, d.act, d.dtype, d.ln_eps = M, Cin, N, Cin, N, L.ACT_NONE, L.PV_BF16, 1e-6
    assert L.lib().pv_ln_linear_rows_supported(C.byref(d)) == 1
    call("pv_ln_linear_rows", d)
    assert rel_err(y, want) <= 1e-2
    y2 = torch.zeros_like(y)
    d.y = y2.data_ptr()
    call("pv_ln_linear_rows", d)
    assert torch.equal(y, y2)
