"""The checks of tests/test_gpu_stencil_kernels.py can fail: each family's check is fed its own float64 reference cast to the
output dtype (it passes), then defective copies of it -- a tap dropped at one corner voxel, the shared (w_mod) filter of a
head taken one chunk over, the fused producer's halo filled with act(pw_shift) instead of zero, a tile missing from psum, a
prefix row shifted by one, LayerNorm statistics over round_up(head_dim, 16) channels, a non-zero padding channel, a touched
canary -- and must raise on each.  No GPU: the references and checks of gpu_util.py are CPU code.  The last test pins a
route predicate that needs no memory: pv_dwconv3d_psum_blocks reads no pointer."""
import ctypes as C

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U

DTYPES = [torch.float32, torch.bfloat16]
K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)


def _dw_cases(dtype):
    return {
        "plain": U.make_dwconv(dtype, 2, 3, 5, 6, 20, (1, 3, 3), S1, (0, 1, 1), L.ACT_SWISH),
        "strided": U.make_dwconv(dtype, 2, 4, 7, 9, 53, K3, (2, 2, 2), P1, L.ACT_RELU, ldx=64, ldy=72),
        "grouped": U.make_dwconv(dtype, 1, 2, 3, 3, 16, K3, S1, P1, L.ACT_RELU, gw=8),
        "qkv_prefix": U.make_dwconv(dtype, 2, 2, 4, 4, 32, K3, (1, 2, 2), P1, L.ACT_NONE, w_mod=16, n_prefix=1, ldy=40, qkv=True),
    }


def _pwdw_case(pw_act=L.ACT_RELU):
    return U.make_pwdw(2, 2, 5, 9, 24, 21, 1, L.ACT_SWISH, pw_act, wide_ldx=True)


def _tp_case(dtype, hd=8, **kw):
    return U.make_token_pool(dtype, 2, 3, hd, (2, 4, 4), K3, [(1, 1, 1), (1, 2, 2)], 1, wide=True, gap=16, **kw)


def _expectations(dtype):
    """name -> (Expect, check(got)) of every family, on its smallest shapes."""
    out = {}
    for name, (i, p) in _dw_cases(dtype).items():
        out["dw_" + name] = (U.expect_dwconv(i, p)[0], lambda got, i=i, p=p: U.check_dwconv(got, i, p))
    if dtype == torch.bfloat16:
        i, p = _pwdw_case()
        out["pwdw"] = (U.expect_pwdw(i, p)[0], lambda got, i=i, p=p: U.check_dwconv(got, i, p))
    for name, kw in (("tp", {}), ("tp_plain", dict(gamma=False, beta=False)), ("tp_gamma", dict(beta=False))):
        i, p = _tp_case(dtype, **kw)
        for z in range(p["n"]):
            out["%s%d" % (name, z)] = (U.expect_token_pool(i, p, z),
                                       lambda got, i=i, p=p, z=z: U.expect_token_pool(i, p, z).check(got, "pv_token_pool"))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_check_passes_on_its_own_reference_and_sees_a_touched_canary(dtype):
    for name, (e, check) in _expectations(dtype).items():
        ideal = e.ideal()
        check(ideal)
        untouched = e.before.clone()
        e._rows(untouched)[..., :e.written][e.owned] = 0
        rest = (untouched == U.CANARY).nonzero()
        assert len(rest), name                              # every case has a stride wider than its rows and a batch gap
        for where in (rest[0], rest[-1]):                   # beyond the padding of the first row; the last gap element
            bad = ideal.clone()
            bad[tuple(where)] = 0.5
            with pytest.raises(AssertionError, match="does not own"):
                check(bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_zero_padding_channel_is_seen(dtype):
    seen = 0
    for name, (e, check) in _expectations(dtype).items():
        if e.written == e.C:
            continue                                        # heads * head_dim and the qkv slice are whole chunks
        bad = e.ideal()
        e._rows(bad)[e.B - 1, e.R - 1, e.C] = 2.0 ** -10
        with pytest.raises(AssertionError, match="padding channels"):
            check(bad)
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["plain", "strided", "qkv_prefix"])
def test_a_tap_dropped_at_one_corner_voxel_is_seen(name, dtype):
    """The last output voxel of the last item loses its centre tap (the one tap of a corner window that is always inside)."""
    i, p = _dw_cases(dtype)[name]
    To, Ho, Wo = U.conv_out_dims(p)
    bad = U.expect_dwconv(i, p, drop=(p["B"] - 1, To - 1, Ho - 1, Wo - 1, p["p"]))[0].ideal()
    with pytest.raises(AssertionError, match="abs-max"):
        U.check_dwconv(bad, i, p)


def test_a_tap_dropped_from_the_fused_producer_and_the_token_pool_is_seen():
    i, p = _pwdw_case()
    To, Ho, Wo = U.conv_out_dims(p)
    with pytest.raises(AssertionError, match="abs-max"):
        U.check_dwconv(U.expect_pwdw(i, p, drop=(1, To - 1, Ho - 1, Wo - 1, (1, 1, 1)))[0].ideal(), i, p)
    for dtype in DTYPES:
        i, p = _tp_case(dtype)
        To, Ho, Wo = U.token_pool_out_dims(p, 1)
        bad = U.expect_token_pool(i, p, 1, drop=(1, To - 1, Ho - 1, Wo - 1, (1, 1, 1))).ideal()
        with pytest.raises(AssertionError, match="abs-max"):
            U.check_token_pool([U.expect_token_pool(i, p, 0).ideal(), bad], i, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_shared_filter_taken_from_the_neighbouring_head_is_seen(dtype):
    i, p = _dw_cases(dtype)["qkv_prefix"]
    with pytest.raises(AssertionError, match="abs-max"):
        U.check_dwconv(U.expect_dwconv(i, p, wrong_head=True)[0].ideal(), i, p)


@pytest.mark.parametrize("pw_act", [L.ACT_NONE, L.ACT_RELU])
def test_a_producer_halo_of_act_shift_instead_of_zero_is_seen(pw_act):
    i, p = _pwdw_case(pw_act)
    e, pre = U.expect_pwdw(i, p)
    U.check_dwconv(e.ideal(), i, p)
    bad_e, bad_pre = U.expect_pwdw(i, p, halo_shift=True)
    with pytest.raises(AssertionError, match="abs-max"):
        U.check_dwconv(bad_e.ideal(), i, p)
    psum = _psum_of(bad_pre, p, 3)                          # and its squeeze sums miss the fused producer's bound
    with pytest.raises(AssertionError, match="mean from psum"):
        U.check_psum(psum, pre, p, 3, U.PSUM_TOL_FUSED)


def _psum_of(pre, p, nblk):
    """Partial sums a kernel would leave: the voxels dealt round-robin to nblk blocks, one block of NaN behind the last."""
    B, S3, Cc = pre.shape
    psum = torch.full((B * nblk + 1, U.round_up8(Cc)), float("nan"))
    body = psum[:B * nblk].view(B, nblk, -1)
    body[:] = 0
    for blk in range(nblk):
        body[:, blk, :Cc] = pre[:, blk::nblk].sum(1).float()
    return psum


@pytest.mark.parametrize("dtype", DTYPES)
def test_psum_check_sees_a_missing_tile_an_unwritten_entry_a_padding_channel_and_an_overrun(dtype):
    i, p = _dw_cases(dtype)["strided"]
    pre = U.expect_dwconv(i, p)[1]
    good = _psum_of(pre, p, 4)
    assert U.check_psum(good, pre, p, 4, U.PSUM_TOL) < 1e-6
    bad = good.clone()
    bad[4 + 2] = 0                                           # one tile's sums never arrive
    with pytest.raises(AssertionError, match="mean from psum"):
        U.check_psum(bad, pre, p, 4, U.PSUM_TOL)
    bad = good.clone()
    bad[4 + 3, 5] = float("nan")
    with pytest.raises(AssertionError, match="not written"):
        U.check_psum(bad, pre, p, 4, U.PSUM_TOL)
    bad = good.clone()
    bad[1, p["C"]] = 2.0 ** -20
    with pytest.raises(AssertionError, match="padding channels of psum"):
        U.check_psum(bad, pre, p, 4, U.PSUM_TOL)
    bad = good.clone()
    bad[8, 0] = 0.0
    with pytest.raises(AssertionError, match="behind the last"):
        U.check_psum(bad, pre, p, 4, U.PSUM_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_prefix_row_shifted_by_one_is_seen(dtype):
    i, p = _dw_cases(dtype)["qkv_prefix"]
    with pytest.raises(AssertionError, match="bit-exact"):
        U.check_dwconv(U.expect_dwconv(i, p, prefix_from=1)[0].ideal(), i, p)
    for kw, match in ((dict(), "abs-max"), (dict(gamma=False, beta=False), "bit-exact")):
        i, p = _tp_case(dtype, **kw)
        bad = [U.expect_token_pool(i, p, z, prefix_from=1).ideal() for z in range(p["n"])]
        with pytest.raises(AssertionError, match=match):
            U.check_token_pool(bad, i, p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [8, 104])
def test_layernorm_statistics_over_sixteen_lane_width_are_seen(hd, dtype):
    i, p = _tp_case(dtype, hd=hd)
    U.check_token_pool([U.expect_token_pool(i, p, z).ideal() for z in range(p["n"])], i, p)
    bad = [U.expect_token_pool(i, p, z, stat_width=(hd + 15) // 16 * 16).ideal() for z in range(p["n"])]
    with pytest.raises(AssertionError, match="abs-max"):
        U.check_token_pool(bad, i, p)


def test_a_clip_beyond_31_bit_offsets_is_counted_in_generic_blocks_not_plane_tiles():
    """bf16 3x3x3 stride 1: Ti*Hi*Wi*ldx (or the output's) above 0x3fffffff falls back to the generic kernel, whose block
    count ceil(To*Ho*ceil(Wo/4) / (256 / (c_p/8))) is what pv_dwconv3d_psum_blocks must report; one frame fewer fits and
    reports the plane kernel's ceil(Ho/4) * ceil(Wo/16) tiles.  No pointer is read, nothing is allocated."""
    p = dict(B=1, T=16, H=512, W=512, C=256, k=K3, s=S1, p=P1, act=L.ACT_RELU, gw=0, w_mod=0, n_prefix=0, ldx=256, ldy=256,
             x_bs=0, y_bs=0)
    blocks = L.lib().pv_dwconv3d_psum_blocks
    d = U.fill_dw_geometry(L.DwConv3dDesc(), p, torch.bfloat16)
    assert 16 * 512 * 512 * 256 > 0x3fffffff
    assert blocks(C.byref(d)) == 16 * 512 * 128 // 8
    d = U.fill_dw_geometry(L.DwConv3dDesc(), dict(p, T=15), torch.bfloat16)
    assert blocks(C.byref(d)) == 128 * 32
    d = U.fill_dw_geometry(L.DwConv3dDesc(), dict(p, T=15, ldy=288), torch.bfloat16)     # the output alone is too large
    assert 15 * 512 * 512 * 288 > 0x3fffffff and blocks(C.byref(d)) == 15 * 512 * 128 // 8
