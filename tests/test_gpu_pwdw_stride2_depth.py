"""pwdw_plane_kernel at stride 2 against the unfused pair, byte for byte, at every exit of its two-plane, two-set walk.

At stride 2 and KS = 1 (pw_cin <= 32) the walk keeps two input planes in flight: plane p + 2 is requested in front of the stencil
of plane p, p + 1 is converted from the operand set requested one plane earlier, two planes per trip.  What can go wrong is the
bookkeeping of that walk -- which set holds which plane, which LDS buffer a plane lands in, the requests `p + 2` and `p + 3` past
the clip (issued against an empty buffer resource), the clip's last output plane (stored the stride-2 way, inside the walk), a
clip shorter than the prefetch distance -- and none of it shows at T = 1 and 3 alone, the only stride-2 clips of
test_gpu_pwdw_bits.py.  Method and helpers are that file's: the fused launch must leave the bytes of pv_conv3d (conv_a into a
dense buffer) followed by pv_dwconv3d, in every byte of the y buffer, the canary gaps between the clips included, and in the
squeeze-excitation sums.  There is no tolerance, and the result does not depend on the commit: the one-plane walk passes too.

Shapes: stride 2 from 10 x 26 and 9 x 25 inputs (even and odd grids, ragged right edge, column tiles that end in the dump row);
T = 1, 2, 3, 4, 5 (shorter than the prefetch distance, both parities of the trip, both guards past the clip); B = 2 with a gap;
pw_cin 24 (KS 1) with C = 53 and 24; act_a RELU and NONE and sums on and off (the four copies of the walk, each met at every T
and tile width), ACT NONE and SWISH; NW = 4 and NW = 2; one pw_cin 40 (KS 2, one plane in flight) case per T.  The fused launch
chooses its tile width by Wo alone (4 from Wo = 12), so the NW = 2 cases come from 10 x 18 and 9 x 17 inputs (Wo = 9, the
second tile ragged); the dw_wide_min_wo knob gives the unfused depthwise launch of the reference the same width, hence the
same tiles and the same sums per block.
PWDW_BITS_RECORD=<file> appends one line per case (the figures of profiles/r36/bits_vs_parent.md)."""
import ctypes as C
import os

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel
from test_gpu_stencil_kernels import WIDE_DEFAULT, _dev, _dw_desc, _plane_blocks
from test_gpu_pwdw_bits import _psum_buf, _same_bytes, _unfused

pytestmark = pytest.mark.gpu

GRIDS = {4: [(10, 26), (9, 25)], 2: [(10, 18), (9, 17)]}      # by tile width NW: Wo = 13 and 9
CLIPS = [1, 2, 3, 4, 5]
# (grid, T, act_a is ReLU, NW, pw_cin)
CASES = [(g, T, r, nw, 24) for g in range(2) for T in CLIPS for r in range(2) for nw in (4, 2)] + [(T % 2, T, T % 2, 4, 40) for T in CLIPS]


def _case(g, T, r, nw, cin):
    H, W = GRIDS[nw][g]
    return dict(H=H, W=W, T=T, cin=cin, NW=nw, pw_act=(L.ACT_NONE, L.ACT_RELU)[r], Cc=53 if (g + T + nw // 4) % 2 else 24,
                act=L.ACT_SWISH if (T + r) % 2 else L.ACT_NONE, sums=(g + r + nw // 4) % 2 == 0)


def test_cases_reach_every_copy_of_the_walk_at_every_clip_length_and_width():
    ks1 = [_case(*x) for x in CASES if x[4] == 24]
    assert {(c["T"], c["NW"], c["pw_act"], c["sums"]) for c in ks1} == {(T, nw, a, s) for T in CLIPS for nw in (4, 2)
                                                                        for a in (L.ACT_NONE, L.ACT_RELU) for s in (False, True)}
    assert {(c["T"], c["H"]) for c in ks1} == {(T, h) for T in CLIPS for h in (10, 9)}
    assert {(c["Cc"], c["act"]) for c in ks1} == {(cc, a) for cc in (24, 53) for a in (L.ACT_NONE, L.ACT_SWISH)}
    assert sorted(c["T"] for c in (_case(*x) for x in CASES if x[4] == 40)) == CLIPS


@pytest.mark.parametrize("g,T,r,nw,cin", CASES)
def test_stride2_fused_launch_leaves_the_bytes_of_the_unfused_pair(g, T, r, nw, cin):
    c = _case(g, T, r, nw, cin)
    i, p = U.make_pwdw(2, T, c["H"], c["W"], cin, c["Cc"], 2, c["act"], c["pw_act"], wide_ldx=(g + T + r) % 2 == 1)
    assert U.conv_out_dims(p) == (T, 5, 13 if nw == 4 else 9)
    nblk = _plane_blocks(p, nw)
    assert nblk != _plane_blocks(p, 6 - nw)       # the block count tells the two tile widths apart
    try:
        L.tune(dw_wide_min_wo=1 if nw == 4 else 1 << 30)   # the unfused depthwise launch too: the same tiles, the same sums per block
        t = _dev(i)
        psum = _psum_buf(p, nblk) if c["sums"] else None
        d = _dw_desc(t, p, torch.bfloat16, psum)
        assert L.lib().pv_dwconv3d_pw_supported(C.byref(d)) == 1 and L.lib().pv_dwconv3d_psum_blocks(C.byref(d)) == nblk
        routed = _routed_kernel(L.OP_DWCONV3D, _dw_desc(_dev(i), p, torch.bfloat16, None if psum is None else _psum_buf(p, nblk)))
        assert "pwdw_plane_kernel" in routed, routed
        call("pv_dwconv3d", d)
        want, want_psum = _unfused(i, p, nblk, c["sums"])
    finally:
        L.tune(dw_wide_min_wo=WIDE_DEFAULT)
    y_same = _same_bytes(t["y0"], want)
    y_err = U.rel_err(t["y0"], want)
    ps_same = None if psum is None else _same_bytes(psum, want_psum)
    line = "S 2 %dx%d T %d NW %d C %d pw_cin %d act_a %d ACT %d sums %s: y %s (max rel %.3e), sums %s" % (
        c["H"], c["W"], T, nw, c["Cc"], cin, c["pw_act"], c["act"], c["sums"], "byte-equal" if y_same else "DIFFER", y_err,
        "-" if ps_same is None else "byte-equal" if ps_same else "DIFFER")
    print(line)
    if os.environ.get("PWDW_BITS_RECORD"):
        with open(os.environ["PWDW_BITS_RECORD"], "a") as f:
            f.write(line + "\n")
    assert y_same, line
    assert ps_same is not False, line
