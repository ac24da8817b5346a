"""pwdw_plane_kernel against the unfused pair, byte for byte.

The fused launch (pv_dwconv3d with pw_w: conv_a + BN + act_a computed per halo tile in front of the depthwise 3x3x3) rounds the
expanded tensor to bf16 exactly where the unfused path stores it, so both must leave the same bytes in y: pv_conv3d (conv_a into
a dense buffer) followed by pv_dwconv3d on that buffer is the reference, two kernels that share no code with the fused one.
Every byte of the y buffer is compared, the canary gaps between the clips included.  The squeeze-excitation sums are compared
byte for byte as well: both kernels add the same fp32 values in the same order (lane, then 16 / 32 lane shuffles, then rows).

Shapes: the smallest that reach every path of the plane walk at NW = 4 -- B = 2 with a gap between the clips; C = 53 (idle
channel pairs, a ragged second slab) and 24; pw_cin 24 (KS 1) and 40 (KS 2, ragged K tail); act_a RELU and NONE, sums on and off
(the four copies of the walk), ACT NONE and SWISH; stride 1 at 5 x 13 with T = 1, 2, 3, 4 (both exits of the two-plane walk);
stride 2 from 10 x 26 and 9 x 25 inputs with T = 1 and 3 (even and odd grids, ragged right edge, column tiles that end in the
dump row).  C, ACT and the sums alternate over geometry x pw_cin x act_a so that every <S, KS> meets every flag pair.
PWDW_BITS_RECORD=<file> appends one line per case (the figures of profiles/r28/bits_vs_parent.md)."""
import ctypes as C
import os

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel
from test_gpu_stencil_kernels import WIDE_DEFAULT, _dev, _dw_desc, _plane_blocks

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 5, 13, 1), (1, 5, 13, 2), (1, 5, 13, 3), (1, 5, 13, 4), (2, 10, 26, 1), (2, 10, 26, 3), (2, 9, 25, 1), (2, 9, 25, 3)]
CASES = [(g, k, r) for g in range(len(GEOMETRY)) for k in range(2) for r in range(2)]


def _case(g, k, r):
    S, H, W, T = GEOMETRY[g]
    return dict(S=S, H=H, W=W, T=T, cin=(24, 40)[k], pw_act=(L.ACT_NONE, L.ACT_RELU)[r], Cc=53 if (g + k) % 2 else 24,
                act=L.ACT_SWISH if (g + r) % 2 else L.ACT_NONE, sums=(g // 2 + k + r) % 2 == 0)


def test_cases_reach_every_copy_of_the_walk():
    seen = {(c["S"], c["cin"], c["pw_act"], c["sums"]) for c in (_case(*x) for x in CASES)}
    assert len(seen) == 2 * 2 * 2 * 2
    assert {(c["S"], c["Cc"], c["act"]) for c in (_case(*x) for x in CASES)} == {(s, cc, a) for s in (1, 2) for cc in (24, 53)
                                                                                 for a in (L.ACT_NONE, L.ACT_SWISH)}


def _psum_buf(p, nblk):
    return torch.full((p["B"] * nblk + 1, U.round_up8(p["C"])), float("nan"), device="cuda")


def _unfused(i, p, nblk, sums):
    """pv_conv3d (conv_a) into a dense buffer, then pv_dwconv3d on it -> (y buffer, sums | None)"""
    B, T, H, W, Cc, cin = p["B"], p["T"], p["H"], p["W"], p["C"], p["pw_cin"]
    cp, cinp = U.round_up8(Cc), U.round_up8(cin)
    t = _dev(i)
    hbuf = torch.zeros(B, T * H * W * cp, dtype=torch.bfloat16, device="cuda")
    wa8 = torch.zeros(Cc, cinp, dtype=torch.bfloat16, device="cuda")
    wa8[:, :cin] = t["wa"]
    c = L.Conv3dDesc()
    c.x, c.w, c.y, c.scale, c.shift = t["x"].data_ptr(), wa8.data_ptr(), hbuf.data_ptr(), t["pw_scale"].data_ptr(), t["pw_shift"].data_ptr()
    c.x_bs, c.y_bs, c.ldx, c.ldy = p["x_bs"], T * H * W * cp, p["ldx"], cp
    c.B, c.Ti, c.Hi, c.Wi, c.cin, c.To, c.Ho, c.Wo, c.cout = B, T, H, W, cinp, T, H, W, Cc
    c.kt = c.kh = c.kw = c.st = c.sh = c.sw = 1
    c.act, c.a_act, c.dtype = p["pw_act"], L.ACT_NONE, L.PV_BF16
    call("pv_conv3d", c)
    q = dict(p, pw_cin=0, pw_act=0, ldx=cp, x_bs=T * H * W * cp)
    t["x"] = hbuf
    psum = _psum_buf(p, nblk) if sums else None
    d = _dw_desc(t, q, torch.bfloat16, psum)
    assert L.lib().pv_dwconv3d_psum_blocks(C.byref(d)) == nblk
    call("pv_dwconv3d", d)
    return t["y0"], psum


def _same_bytes(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("g,k,r", CASES)
def test_fused_launch_leaves_the_bytes_of_the_unfused_pair(g, k, r):
    c = _case(g, k, r)
    i, p = U.make_pwdw(2, c["T"], c["H"], c["W"], c["cin"], c["Cc"], c["S"], c["act"], c["pw_act"], wide_ldx=(g + k + r) % 2 == 1)
    assert U.conv_out_dims(p)[1:] == (5, 13)
    nblk = _plane_blocks(p, 4)
    try:
        L.tune(dw_wide_min_wo=1)      # NW = 4 for the unfused depthwise launch too: the same tiles, the same sums per block
        t = _dev(i)
        psum = _psum_buf(p, nblk) if c["sums"] else None
        d = _dw_desc(t, p, torch.bfloat16, psum)
        assert L.lib().pv_dwconv3d_pw_supported(C.byref(d)) == 1 and L.lib().pv_dwconv3d_psum_blocks(C.byref(d)) == nblk
        routed = _routed_kernel(L.OP_DWCONV3D, _dw_desc(_dev(i), p, torch.bfloat16, None if psum is None else _psum_buf(p, nblk)))
        assert "pwdw_plane_kernel" in routed and nblk != _plane_blocks(p, 2), routed      # the block count is NW = 4's
        call("pv_dwconv3d", d)
        want, want_psum = _unfused(i, p, nblk, c["sums"])
    finally:
        L.tune(dw_wide_min_wo=WIDE_DEFAULT)
    y_same = _same_bytes(t["y0"], want)
    y_err = U.rel_err(t["y0"], want)
    ps_same = None if psum is None else _same_bytes(psum, want_psum)
    line = "S %d %dx%d T %d C %d pw_cin %d act_a %d ACT %d sums %s: y %s (max rel %.3e), sums %s" % (
        c["S"], c["H"], c["W"], c["T"], c["Cc"], c["cin"], c["pw_act"], c["act"], c["sums"], "byte-equal" if y_same else "DIFFER", y_err,
        "-" if ps_same is None else "byte-equal" if ps_same else "DIFFER")
    if ps_same is False:
        a, b = psum.float().cpu(), want_psum.float().cpu()
        diff = torch.nan_to_num(a - b)
        idx = diff.abs().flatten().argmax().item()
        line += " (%d entries, max |d| %.3e of %.3e at row %d col %d)" % (
            (diff != 0).sum().item(), diff.abs().max().item(), b.flatten()[idx].abs().item(), idx // a.shape[1], idx % a.shape[1])
    print(line)
    if os.environ.get("PWDW_BITS_RECORD"):
        with open(os.environ["PWDW_BITS_RECORD"], "a") as f:
            f.write(line + "\n")
    assert y_same, line
    assert ps_same is not False, line
