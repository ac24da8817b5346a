"""The checks of tests/test_gpu_misc_kernels.py can fail: each family's check is fed its own float64 reference cast to the
output dtype (it passes), then defective copies of it -- a tap dropped from one corner window of a pool, the gamma / beta
row of one LayerNorm row taken from the neighbouring period, one padding channel non-zero, a canary overwritten -- and
must raise on each.  No GPU: the references and checks of gpu_util.py are CPU code."""
import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U

DTYPES = [torch.float32, torch.bfloat16]


def _cases(dtype):
    """family -> (expectation, check, inputs, params) on small shapes of every family."""
    out = {}
    for name, make, expect, check in [
        ("softmax", lambda: U.make_softmax(dtype, 5, 65, False), U.expect_softmax, U.check_softmax),
        ("softmax_inplace", lambda: U.make_softmax(dtype, 5, 65, True), U.expect_softmax, U.check_softmax),
        ("mean", lambda: U.make_mean(dtype, 3, 7, 20), U.expect_mean, U.check_mean),
        ("posenc", lambda: U.make_posenc(dtype, "sep_cls_posclass", 20, 32), U.expect_posenc, U.check_posenc),
        ("posenc_full", lambda: U.make_posenc(dtype, "full_cls", 20, 32), U.expect_posenc, U.check_posenc),
        ("posenc_cls_only", lambda: U.make_posenc(dtype, "sep_cls", 20, 32, cls_only=1), U.expect_posenc, U.check_posenc),
        ("add_act", lambda: U.make_add_act(dtype, 9, 20, L.ACT_GELU, False), U.expect_add_act, U.check_add_act),
        ("pool_max", lambda: U.make_pool(dtype, 2, 4, 5, 5, 20, (3, 3, 3), (1, 2, 2), (1, 1, 1), L.POOL_MAX, 1, 16), U.expect_pool, U.check_pool),
        ("pool_avg", lambda: U.make_pool(dtype, 2, 4, 5, 5, 20, (3, 3, 3), (1, 2, 2), (1, 1, 1), L.POOL_AVG, 1, 16), U.expect_pool, U.check_pool),
        ("layernorm", lambda: U.make_layernorm(dtype, 37, 20, g_period=8), U.expect_layernorm, U.check_layernorm),
        ("layernorm_f32in", lambda: U.make_layernorm(torch.bfloat16, 9, 20, x_f32=True), U.expect_layernorm, U.check_layernorm),
        ("affine", lambda: U.make_affine(dtype, 12, 20, False, True, L.ACT_GELU, 1, 4), U.expect_affine, U.check_affine),
        ("affine_out", lambda: U.make_affine(dtype, 12, 20, False, False, L.ACT_RELU, 1, 4), U.expect_affine, U.check_affine),
        ("ingest", lambda: U.make_ingest(torch.float32, dtype, 11, 3, 5, 16, 24, False), U.expect_ingest, U.check_ingest),
        ("ingest_affine", lambda: U.make_ingest(torch.uint8, dtype, 11, 3, 5, 16, 24, True), U.expect_ingest, U.check_ingest),
        ("ingest_c4", lambda: U.make_ingest(torch.uint8, torch.bfloat16, 3, 3, 5, 4, 4, True), U.expect_ingest, U.check_ingest),
        ("egress", lambda: U.make_egress(torch.float32, dtype), U.expect_egress, U.check_egress),
    ]:
        i, p = make()
        out[name] = (expect(i, p), check, i, p)
    if dtype == torch.float32:
        i, p = U.make_se_gate(2, 20, 6, 3, extra_pad=8)
        out["se_gate"] = (U.expect_se_gate(i, p), U.check_se_gate, i, p)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_check_passes_on_its_own_reference_and_sees_a_touched_canary(dtype):
    for name, (e, check, i, p) in _cases(dtype).items():
        ideal = e.ideal()
        check(ideal, i, p)
        # an element the launch does not own: the last one of the buffer (beyond the padding / in the gap), where there is one
        untouched = e.before.clone()
        e._rows(untouched)[..., :e.written][e.owned] = 0
        rest = (untouched == U.CANARY).nonzero()
        if len(rest):
            bad = ideal.clone()
            bad[tuple(rest[-1])] = 0.5
            with pytest.raises(AssertionError, match="does not own"):
                check(bad, i, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_zero_padding_channel_is_seen(dtype):
    seen = 0
    for name, (e, check, i, p) in _cases(dtype).items():
        if e.written == e.C:
            continue                                   # the kernel writes no padding (softmax, mean, egress)
        bad = e.ideal()
        b, r = (int(v) for v in e.owned.nonzero()[-1])
        e._rows(bad)[b, r, e.C] = 2.0 ** -10
        with pytest.raises(AssertionError, match="padding channels"):
            check(bad, i, p)
        seen += 1
    assert seen >= 9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [L.POOL_MAX, L.POOL_AVG])
@pytest.mark.parametrize("k,pad", [((3, 3, 3), (1, 1, 1)), ((4, 4, 4), (0, 0, 0))])
def test_a_tap_dropped_from_one_corner_window_is_seen(k, pad, mode, dtype):
    """The last window of the last item loses its last tap (the far corner of the grid).  For the maximum the far-corner voxel
    is made the window's largest, or dropping it would change nothing."""
    i, p = U.make_pool(dtype, 2, 4, 5, 5, 20, k, (1, 1, 1), pad, mode, n_prefix=1, gap=16)
    To, Ho, Wo = U.pool_out_dims(p)
    rows = i["x"][:, :p["x_bs"] - 16].view(2, -1, p["ldx"])
    rows[1, -1, :20] = 5.0                             # voxel (T-1, H-1, W-1) of item 1
    tap = tuple(kk - 1 - pd for kk, pd in zip(k, pad))  # the tap of the last window that reads it
    U.check_pool(U.expect_pool(i, p).ideal(), i, p)
    bad = U.expect_pool(i, p, drop=(1, To - 1, Ho - 1, Wo - 1, tap)).ideal()
    with pytest.raises(AssertionError, match="bit-exact|abs-max"):
        U.check_pool(bad, i, p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g_period,ramp", [(8, True), (16, False), (2, False)])
def test_a_gamma_row_of_the_neighbouring_period_is_seen(g_period, ramp, dtype):
    i, p = U.make_layernorm(dtype, 67, 24, g_period=g_period, ramp=ramp)
    U.check_layernorm(U.expect_layernorm(i, p).ideal(), i, p)
    bad = U.expect_layernorm(i, p, wrong_row=66).ideal()          # one row, the last: where a second grid trip would land
    with pytest.raises(AssertionError, match="abs-max"):
        U.check_layernorm(bad, i, p)


def test_ensemble_check_passes_on_its_reference_and_sees_a_miscounted_clip():
    for mode in (0, 1):
        i, p = U.make_ensemble(mode)
        e, cnt = U.expect_ensemble(i, p)
        U.check_ensemble((e.ideal().view(p["V"], p["C"]), cnt), i, p)
        with pytest.raises(AssertionError, match="counts"):
            U.check_ensemble((e.ideal().view(p["V"], p["C"]), cnt + torch.tensor([0, 0, 0, 1], dtype=torch.int32)), i, p)
        moved = e.ideal().view(p["V"], p["C"]).clone()
        moved[3, 0] += 2.0 ** -12                                  # the video without a clip must keep its bits
        with pytest.raises(AssertionError, match="bit-exact"):
            U.check_ensemble((moved, cnt), i, p)


def test_softmax_check_sees_rows_that_do_not_sum_to_one():
    i, p = U.make_softmax(torch.float32, 5, 400, False)
    bad = U.expect_softmax(i, p).ideal()
    U.rows_of(bad, 5, p["ldy"], 400)[0, 2] *= 1.02
    with pytest.raises(AssertionError):
        U.check_softmax(bad, i, p)
