"""Statuses of the row, pooling, layout, SE-gate, fused-MLP, LayerNorm + Linear and attention entries for descriptors they reject before any launch: one table of
(entry, change to a valid descriptor, status).  PV_ERR_INVALID is a descriptor that contradicts itself, PV_ERR_UNSUPPORTED
one that is consistent but has no kernel; callers tell them apart, so the table pins which of the two each case gets.
No compute, runs without a GPU: the pointers are addresses of a host buffer that no entry dereferences."""
import ctypes as C

from pytorchvideo_amd import _lib as L

INVALID, UNSUPPORTED = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED
_BUF = C.create_string_buffer(256)
P = (C.addressof(_BUF) + 63) // 64 * 64        # a 64-byte aligned non-null address
NO_DTYPE = 7

# entry -> (descriptor type, a descriptor the entry would launch)
BASE = {
    "pv_se_gate": (L.SeGateDesc, dict(psum=P, gate=P, w1=P, w2=P, B=2, C=20, c_p=24, cr=6, nblk=3, inv_count=0.5)),
    # 3x3x3 window, stride (1, 2, 2), padding 1: 4 x 5 x 5 -> 4 x 3 x 3
    "pv_pool3d": (L.Pool3dDesc, dict(x=P, y=P, x_bs=2400, y_bs=864, ldx=24, ldy=24, B=1, Ti=4, Hi=5, Wi=5, C=20, To=4, Ho=3,
                                     Wo=3, kt=3, kh=3, kw=3, st=1, sh=2, sw=2, pt=1, ph=1, pw=1, mode=L.POOL_MAX,
                                     dtype=L.PV_F32)),
    "pv_ingest_ncdhw": (L.LayoutDesc, dict(src=P, dst=P, B=1, C=3, T=2, H=3, W=5, c_p=16, ld=24, bs=720, src_dtype=L.PV_F32,
                                           dst_dtype=L.PV_BF16)),
    # the 4-channel first-layer layout
    "pv_ingest_ncdhw/c4": (L.LayoutDesc, dict(src=P, dst=P, B=1, C=3, T=2, H=3, W=5, c_p=4, ld=4, bs=120,
                                              src_dtype=L.PV_U8, dst_dtype=L.PV_BF16)),
    "pv_egress_ncdhw": (L.LayoutDesc, dict(src=P, dst=P, B=1, C=3, T=2, H=3, W=5, c_p=16, ld=24, bs=720,
                                           src_dtype=L.PV_BF16, dst_dtype=L.PV_F32)),
}
_ROWS = dict(x=P, y=P, rows=10, C=20, ldx=24, ldy=24, eps=1e-6, dtype=L.PV_F32)
for _e in ("pv_layernorm", "pv_affine_rows", "pv_softmax_rows"):
    BASE[_e] = (L.RowsDesc, _ROWS)
BASE["pv_mean_rows"] = (L.RowsDesc, dict(_ROWS, rows_per_batch=5))
BASE["pv_add_posenc"] = (L.PosencDesc, dict(x=P, pos_spatial=P, B=1, T=2, HW=4, C=20, ld=24, dtype=L.PV_F32))
BASE["pv_add_act"] = (L.AddDesc, dict(a=P, b=P, y=P, rows=5, C=20, lda=24, ldb=24, ldy=24, dtype=L.PV_F32))
BASE["pv_ensemble_scores"] = (L.EnsembleDesc, dict(logits=P, video_index=P, accum=P, counts=P, N=3, C=10, ld=16, V=2, mode=0))
# csrc/pv_mlp.hip: operand mode (bf16 x, residual, b2), LayerNorm mode (fp32 x, C == Cout, no residual), operand mode with yn
_MLP = dict(x=P, w12=P, y=P, b2=P, M=10, C=96, H=64, Cout=192, ldx=96, ldy=192, act=L.ACT_GELU, dtype=L.PV_BF16)
BASE["pv_mlp_rows"] = (L.MlpDesc, dict(_MLP, residual=P, ldr=192))
BASE["pv_mlp_rows/ln"] = (L.MlpDesc, dict(_MLP, Cout=96, ldy=96, ln_gamma=P, ln_beta=P, ln_eps=1e-6))
BASE["pv_mlp_rows/yn"] = (L.MlpDesc, dict(_MLP, yn=P, nn_gamma=P, nn_beta=P, ldyn=192, nn_eps=1e-6))
BASE["pv_ln_linear_rows"] = (L.LnLinearDesc, dict(x=P, wb=P, y=P, ln_gamma=P, ln_beta=P, M=10, C=96, N=64, ldx=96, ldy=64,
                                                  dtype=L.PV_BF16, ln_eps=1e-6))
# csrc/pv_attn.hip: 2 items x 7 rows of 2 heads x 32 channels; K / V 5 rows
_ATTN = dict(q=P, k=P, v=P, o=P, B=2, heads=2, head_dim=32, Nq=7, Nk=5, ldq=64, ldk=64, ldv=64, ldo=64, q_bs=448, k_bs=320, v_bs=320,
             o_bs=448, scale=0.125)
BASE["pv_attention"] = (L.AttentionDesc, dict(_ATTN, dtype=L.PV_BF16))
BASE["pv_attention/f32"] = (L.AttentionDesc, dict(_ATTN, dtype=L.PV_F32))
SUPPORTED = {"pv_mlp_rows": "pv_mlp_rows_supported", "pv_ln_linear_rows": "pv_ln_linear_rows_supported"}


def _each(entry, status, **values):
    """One row per (field, value): every change alone."""
    return [(entry, {k: v}, status) for k, vs in values.items() for v in (vs if isinstance(vs, tuple) else (vs,))]


TABLE = (
    [(e, None, INVALID) for e in BASE]                                    # no descriptor at all
    # ---- pv_se_gate
    + _each("pv_se_gate", INVALID, psum=None, gate=None, w1=None, w2=None, B=0, C=(0, -1), cr=0, nblk=0,
            c_p=(16, 25))                                                 # c_p < C; c_p no multiple of 8
    # ---- pv_pool3d
    + _each("pv_pool3d", INVALID, x=None, y=None, B=0, C=0, To=(0, 5), Ho=(0, 4), Wo=(0, 2),   # zero / not what the window gives
            ldx=20, ldy=20, x_bs=2404, y_bs=868, kt=0, kh=0, kw=0, st=0, sh=0, sw=0, mode=(2, -1))
    + _each("pv_pool3d", UNSUPPORTED, dtype=(NO_DTYPE, L.PV_U8))
    + [("pv_pool3d", dict(mode=2, dtype=NO_DTYPE), INVALID)]              # the mode is checked before the dtype
    # ---- pv_ingest_ncdhw, generic layout
    + _each("pv_ingest_ncdhw", INVALID, src=None, dst=None, B=0, C=0, T=0, H=0, W=0, c_p=(12, 0), ld=(20, 8), bs=724)
    + [("pv_ingest_ncdhw", dict(t_index=P, src_T=0), INVALID),
       ("pv_ingest_ncdhw", dict(t_index=P, src_T=0, src_dtype=NO_DTYPE), INVALID)]
    + _each("pv_ingest_ncdhw", UNSUPPORTED, src_dtype=(NO_DTYPE, L.PV_U16), dst_dtype=(NO_DTYPE, L.PV_U8))
    # ---- pv_ingest_ncdhw, 4-channel layout; a descriptor that is not quite one falls through to the generic check
    + [("pv_ingest_ncdhw/c4", dict(t_index=P, src_T=0), INVALID),
       ("pv_ingest_ncdhw/c4", dict(t_index=P, src_T=0, src_dtype=NO_DTYPE), INVALID),
       ("pv_ingest_ncdhw/c4", dict(src_dtype=NO_DTYPE), UNSUPPORTED),
       ("pv_ingest_ncdhw/c4", dict(src_dtype=NO_DTYPE, H=4, W=4, bs=128), UNSUPPORTED),   # the 8-voxel form's geometry
       ("pv_ingest_ncdhw/c4", dict(bs=122), INVALID),                     # bs % 4 != 0
       ("pv_ingest_ncdhw/c4", dict(dst_dtype=L.PV_F32), INVALID),
       ("pv_ingest_ncdhw/c4", dict(C=5), INVALID),
       ("pv_ingest_ncdhw/c4", dict(ld=8), INVALID),
       ("pv_ingest_ncdhw/c4", dict(B=0), INVALID),
       ("pv_ingest_ncdhw/c4", dict(src=None), INVALID)]
    # ---- pv_egress_ncdhw
    + _each("pv_egress_ncdhw", INVALID, src=None, dst=None, B=0, C=0, T=0, H=0, W=0, c_p=(12, 4, 0), ld=(20, 8), bs=724)
    + _each("pv_egress_ncdhw", UNSUPPORTED, src_dtype=(NO_DTYPE, L.PV_U8), dst_dtype=(NO_DTYPE, L.PV_U8))
    # ---- pv_layernorm
    + _each("pv_layernorm", INVALID, x=None, y=None, rows=0, C=0, ldx=20, ldy=20, g_period=(17, -1))
    + _each("pv_layernorm", UNSUPPORTED, g_period=(3, 5), dtype=NO_DTYPE)
    + [("pv_layernorm", dict(g_period=8, x_f32=1, dtype=L.PV_BF16), UNSUPPORTED),
       ("pv_layernorm", dict(g_period=8, C=264, ldx=264, ldy=264), UNSUPPORTED),          # 33 chunks: beyond the narrow-row kernel
       ("pv_layernorm", dict(g_period=17, x_f32=1, dtype=L.PV_BF16), INVALID)]
    + [("pv_layernorm", dict(C=2056, ldx=2056, ldy=2056, dtype=dt, x_f32=xf), UNSUPPORTED)  # 257 chunks
       for dt, xf in ((L.PV_F32, 0), (L.PV_BF16, 0), (L.PV_BF16, 1), (NO_DTYPE, 0))]
    # ---- pv_affine_rows
    + _each("pv_affine_rows", INVALID, x=None, y=None, rows=0, C=0, ldx=20, ldy=20, g_period=1, n_prefix=(-1, 1),
            rows_per_batch=-1)                                            # n_prefix = 1 without rows_per_batch
    + _each("pv_affine_rows", UNSUPPORTED, dtype=(NO_DTYPE, L.PV_U8))
    # ---- pv_softmax_rows
    + _each("pv_softmax_rows", INVALID, x=None, y=None, rows=(0, -1), C=0)
    + _each("pv_softmax_rows", UNSUPPORTED, dtype=NO_DTYPE)
    # ---- pv_mean_rows
    + _each("pv_mean_rows", INVALID, x=None, y=None, rows=0, C=0, rows_per_batch=(0, -1, 3, 20))   # 10 % 3, 10 % 20
    + _each("pv_mean_rows", UNSUPPORTED, dtype=NO_DTYPE)
    # ---- pv_add_posenc
    + _each("pv_add_posenc", INVALID, x=None, pos_spatial=None, B=0, T=0, HW=0, C=0, ld=20, cls_only=1)   # no cls_token
    + _each("pv_add_posenc", UNSUPPORTED, dtype=NO_DTYPE)
    + [("pv_add_posenc", dict(cls_only=1, dtype=NO_DTYPE), INVALID)]
    # ---- pv_add_act
    + _each("pv_add_act", INVALID, a=None, b=None, y=None, rows=0, C=0, lda=20, ldb=20, ldy=20)
    + _each("pv_add_act", UNSUPPORTED, dtype=NO_DTYPE)
    # ---- pv_ensemble_scores
    + _each("pv_ensemble_scores", INVALID, logits=None, video_index=None, accum=None, counts=None, N=0, C=0, V=0, ld=8,
            mode=(2, -1))
    # ---- pv_mlp_rows (check() of csrc/pv_mlp.hip, then the (C, Cout) table of the entry)
    + _each("pv_mlp_rows", INVALID, x=None, w12=None, y=None, M=(0, -1, 0x80000000),
            ldx=(88, 100), ldy=(184, 194), ldr=(184, 194))                # too small; bf16 rows of 8, fp32 rows of 4 elements
    + _each("pv_mlp_rows", UNSUPPORTED, dtype=(NO_DTYPE, L.PV_F32), C=(0, 80), H=(0, 48), Cout=(0, 200))
    + [("pv_mlp_rows", dict(C=768, ldx=768), UNSUPPORTED),                # consistent, but no (C, Cout) instantiation
       ("pv_mlp_rows", dict(C=384, ldx=384), UNSUPPORTED),
       ("pv_mlp_rows", dict(C=128, ldx=128), UNSUPPORTED),
       ("pv_mlp_rows", dict(x=None, dtype=NO_DTYPE), INVALID)]            # the pointers are checked before the dtype
    # LayerNorm mode: beta and b2 required, C == Cout, the residual is x itself; fp32 rows of 4 elements
    + _each("pv_mlp_rows/ln", INVALID, ln_beta=None, b2=None, residual=P, ldx=(92, 98), ldy=(88, 98))
    + [("pv_mlp_rows/ln", dict(Cout=192, ldy=192), INVALID),
       ("pv_mlp_rows/ln", dict(C=128, Cout=128, ldx=128, ldy=128), UNSUPPORTED),
       ("pv_mlp_rows/ln", dict(C=768, Cout=768, ldx=768, ldy=768), UNSUPPORTED),
       ("pv_mlp_rows/ln", dict(dtype=L.PV_F32), UNSUPPORTED)]
    # yn needs its parameters and a bf16 row of 8 elements
    + _each("pv_mlp_rows/yn", INVALID, nn_gamma=None, nn_beta=None, ldyn=(0, 184, 196))
    # ---- pv_ln_linear_rows (check_ln_linear(), then the C switch of the entry)
    + _each("pv_ln_linear_rows", INVALID, x=None, wb=None, y=None, M=(0, -1, 0x80000000), ln_gamma=None, ln_beta=None,
            ldx=(92, 98), ldy=(56, 68))
    + _each("pv_ln_linear_rows", UNSUPPORTED, dtype=(NO_DTYPE, L.PV_F32), C=(0, 80), N=(0, 48))
    + [("pv_ln_linear_rows", dict(C=128, ldx=128), UNSUPPORTED),
       ("pv_ln_linear_rows", dict(C=1536, ldx=1536), UNSUPPORTED),
       ("pv_ln_linear_rows", dict(ln_gamma=None, dtype=NO_DTYPE), UNSUPPORTED)]   # the dtype is checked before the parameters
    # ---- pv_attention: pointers, counts, alignment (rows of 8 bf16 / 4 fp32 elements), scale, row width; then head_dim and dtype
    + [(e, {k: v}, INVALID) for e in ("pv_attention", "pv_attention/f32")
       for k, vs in dict(q=None, k=None, v=None, o=None, B=(0, -1), heads=(0, -1), head_dim=(0, -32), Nq=(0, -1), Nk=(0, -1),
                         ldq=56, ldk=56, ldv=56, ldo=56,                  # < heads * head_dim
                         scale=(0.0, -0.125, float("inf"), float("nan"))).items()
       for v in (vs if isinstance(vs, tuple) else (vs,))]
    + _each("pv_attention", INVALID, ldq=68, ldk=68, ldv=68, ldo=68, q_bs=452, k_bs=324, v_bs=324, o_bs=452)       # % 8
    + _each("pv_attention/f32", INVALID, ldq=66, ldk=66, ldv=66, ldo=66, q_bs=450, k_bs=322, v_bs=322, o_bs=450)   # % 4
    + [("pv_attention", dict(head_dim=40, ldq=80, ldk=80, ldv=80, ldo=80), UNSUPPORTED),
       ("pv_attention/f32", dict(head_dim=40, ldq=80, ldk=80, ldv=80, ldo=80), UNSUPPORTED),
       ("pv_attention", dict(dtype=NO_DTYPE), UNSUPPORTED),
       ("pv_attention", dict(dtype=L.PV_U8), UNSUPPORTED),
       ("pv_attention", dict(dtype=NO_DTYPE, ldq=68), UNSUPPORTED),       # an unknown dtype is held to rows of 4 elements ...
       ("pv_attention", dict(dtype=NO_DTYPE, ldq=66), INVALID),           # ... and the alignment is checked before the dtype
       ("pv_attention", dict(head_dim=40), INVALID),                      # the row width (ld 64 < 2 * 40) before the head_dim
       ("pv_attention", dict(dtype=NO_DTYPE, scale=0.0), INVALID),
       ("pv_attention", dict(q=None, head_dim=40), INVALID)]
)


def test_every_rejected_descriptor_gets_its_status(pv_lib):
    wrong = []
    for entry, change, status in TABLE:
        cls, base = BASE[entry]
        fn = getattr(pv_lib, entry.split("/")[0])
        got = fn(None, None) if change is None else fn(C.byref(cls(**dict(base, **change))), None)
        if got != status:
            wrong.append("%s %s: status %d, expected %d" % (entry, change, got, status))
    assert not wrong, "\n".join(wrong)


def test_the_supported_queries_are_zero_exactly_where_the_launch_declines(pv_lib):
    """pv_mlp_rows_supported / pv_ln_linear_rows_supported: 1 for the descriptors the entries would launch, 0 for every row of
    the table (whichever of the two statuses the launch gives) and for no descriptor at all."""
    wrong = []
    for entry, (cls, base) in BASE.items():
        if entry.split("/")[0] in SUPPORTED and getattr(pv_lib, SUPPORTED[entry.split("/")[0]])(C.byref(cls(**base))) != 1:
            wrong.append("%s: its base descriptor is not supported" % entry)
    rows = 0
    for entry, change, status in TABLE:
        if entry.split("/")[0] not in SUPPORTED:
            continue
        cls, base = BASE[entry]
        q = getattr(pv_lib, SUPPORTED[entry.split("/")[0]])
        got = q(None) if change is None else q(C.byref(cls(**dict(base, **change))))
        rows += 1
        if got != 0 or status >= 0:
            wrong.append("%s %s: supported says %d, the launch status is %d" % (entry, change, got, status))
    assert rows > 60 and not wrong, "\n".join(wrong)
