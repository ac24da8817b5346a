"""Helpers for the -m gpu tests: raw C-ABI calls on torch-owned device memory."""
import ctypes as C
import math

import torch

from pytorchvideo_amd import _lib as L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pv_dtype(t):
    return L.PV_BF16 if t.dtype == torch.bfloat16 else L.PV_F32


def call(fn_name, desc):
    lib = L.lib()
    L.check(getattr(lib, fn_name)(C.byref(desc), stream()), fn_name)
    torch.cuda.synchronize()


def rel_err(got, want):
    want = want.float().cpu()
    return (got.float().cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-6)


def _routed_kernel(op, d):
    """Symbol of the kernel the library routes descriptor `d` to under the current knobs (a one-op plan, profiled once)."""
    lib = L.lib()
    plan = lib.pv_plan_create()
    try:
        L.check(lib.pv_plan_add(plan, op, C.byref(d), C.sizeof(d)), "pv_plan_add")
        ms = (C.c_float * 1)()
        L.check(lib.pv_plan_profile(plan, C.c_void_p(torch.cuda.current_stream().cuda_stream), 1, ms), "pv_plan_profile")
        return (lib.pv_plan_op_kernel(plan, 0) or b"").decode()
    finally:
        lib.pv_plan_destroy(plan)


# ------------------------------------------------------------------ pv_rows / pv_pool / pv_layout / pv_segate.hip families: float64 references and checks
# Everything below runs on the CPU (tests/test_misc_kernel_checks.py feeds the checks their own reference and defective
# copies of it); tests/test_gpu_misc_kernels.py feeds them what the kernels left on the device.
#
# A buffer is a (B, bs) tensor: item b holds R rows of `ld` elements from its start, the rest of the item is the gap behind
# it.  A launch owns channels [0, written) of the rows it owns; every other element must come back as it went in (the
# canary, or the input of an in-place launch).
CANARY = 7.0
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}
BF16_ROUND = 2.0 ** -8          # one bf16 rounding, relative (tests/test_transforms.py)


def round_up8(c):
    return (c + 7) // 8 * 8


def randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale + shift


def rows_buf(data, ld, dtype, bs=None, written=None):
    """(B, R, C) values -> (B, bs) buffer: channels [C, written) zero, everything else the canary."""
    B, R, Cc = data.shape
    written = round_up8(Cc) if written is None else written
    buf = torch.full((B, bs or R * ld), CANARY, dtype=dtype)
    rows = buf[:, :R * ld].view(B, R, ld)
    rows[..., :Cc] = data.to(dtype)
    rows[..., Cc:written] = 0
    return buf


def rows_of(buf, R, ld, Cc):
    return buf[:, :R * ld].view(buf.shape[0], R, ld)[..., :Cc]


def canary_buf(B, bs, dtype):
    return torch.full((B, bs), CANARY, dtype=dtype)


def _abs_rel(got, want):
    want, got = want.double(), got.double()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-6) if want.numel() else 0.0


class Expect:
    """What one launch must leave in its output buffer.

    want    (B, R, C) reference values (float64; float32 where the kernel's own fp32 order is the reference)
    before  (B, bs) the buffer as it was handed to the launch
    tol     bound on max|got - want| / max|want|; None: every owned row is bit-equal to `want` cast to the buffer's dtype
    per_elem  instead of tol: |got - want| <= per_elem * |want| for every element
    exact   (B, R) bool: rows that are bit-equal even where `tol` is given
    owned   (B, R) bool: rows the launch writes (default all)
    written channels of an owned row the launch writes; [C, written) must be zero (default round_up(C, 8))
    """

    def __init__(self, want, before, ld, tol=None, per_elem=None, exact=None, owned=None, written=None):
        self.want, self.before, self.ld, self.tol, self.per_elem = want.cpu(), before.cpu().clone(), ld, tol, per_elem
        self.B, self.R, self.C = want.shape
        self.written = round_up8(self.C) if written is None else written
        full = torch.ones(self.B, self.R, dtype=torch.bool)
        self.owned = full if owned is None else owned
        self.exact = (full if tol is None and per_elem is None else ~full) if exact is None else exact
        assert self.R * ld <= self.before.shape[1] and self.written <= ld and self.before.shape[0] == self.B

    def _rows(self, buf):
        return buf[:, :self.R * self.ld].view(self.B, self.R, self.ld)

    def ideal(self):
        """The buffer a kernel that computes the reference exactly leaves."""
        buf = self.before.clone()
        rows = self._rows(buf)
        rows[..., :self.C][self.owned] = self.want.to(buf.dtype)[self.owned]
        rows[..., self.C:self.written][self.owned] = 0
        return buf

    def check(self, got, what=""):
        got = got.detach().cpu()
        assert got.shape == self.before.shape and got.dtype == self.before.dtype, what
        g = self._rows(got)
        data, want, ex = g[..., :self.C][self.owned], self.want[self.owned], self.exact[self.owned]
        if ex.any():
            bad = (data[ex] != want[ex].to(got.dtype)).sum().item()
            assert bad == 0, "%s: %d elements of rows that must be bit-exact differ from the reference" % (what, bad)
        err = 0.0
        if (~ex).any():
            d, w = data[~ex].double(), want[~ex].double()
            if self.per_elem is not None:
                err = ((d - w).abs() / w.abs().clamp_min(1e-30)).max().item()
                assert ((d - w).abs() <= self.per_elem * w.abs()).all(), \
                    "%s: worst element-wise relative error %.3e > %.3e" % (what, err, self.per_elem)
            else:
                err = _abs_rel(d, w)
                assert err <= self.tol, "%s: error %.3e of the reference abs-max > %.1e" % (what, err, self.tol)
        pads = g[..., self.C:self.written][self.owned]
        assert (pads == 0).all(), "%s: %d padding channels of written rows are not zero" % (what, (pads != 0).sum().item())
        rest_got, rest_before = got.clone(), self.before.clone()
        self._rows(rest_got)[..., :self.written][self.owned] = 0
        self._rows(rest_before)[..., :self.written][self.owned] = 0
        bad = (rest_got != rest_before).sum().item()
        assert bad == 0, "%s: %d elements the launch does not own (beyond the padding, other rows, gaps) changed" % (what, bad)
        return err


def ref_act(v, act):
    v = v.double()
    if act == L.ACT_RELU:
        return v.clamp_min(0)
    if act == L.ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == L.ACT_GELU:
        return 0.5 * v * (1 + torch.erf(v * 0.5 ** 0.5))
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


# ---- pv_softmax_rows: p = rows, C, ldx, ldy; i = x (1, rows*ldx), y0 (x itself when in place)
def expect_softmax(i, p):
    want = torch.softmax(rows_of(i["x"].cpu(), p["rows"], p["ldx"], p["C"]).double(), -1)
    return Expect(want, i["y0"], p["ldy"], tol=TOL[i["y0"].dtype], written=p["C"])


def check_softmax(got, i, p):
    err = expect_softmax(i, p).check(got, "pv_softmax_rows")
    sums = rows_of(got.cpu(), p["rows"], p["ldy"], p["C"]).double().sum(-1)
    worst = (sums - 1).abs().max().item()
    assert worst <= TOL[got.dtype], "pv_softmax_rows: a row sums to 1 %+.3e" % worst
    return err


# ---- pv_mean_rows: p = rows, rows_per_batch, C, ldx, ldy; i = x (1, rows*ldx), y0 (1, B*ldy) fp32
def expect_mean(i, p):
    x = rows_of(i["x"].cpu(), p["rows"], p["ldx"], p["C"]).double()
    want = x.reshape(-1, p["rows_per_batch"], p["C"]).mean(1)[None]
    return Expect(want, i["y0"], p["ldy"], tol=TOL[i["x"].dtype], written=p["C"])


def check_mean(got, i, p):
    return expect_mean(i, p).check(got, "pv_mean_rows")


# ---- pv_add_posenc: p = B, T, HW, C, ld, cls_only; i = x (1, B*rows*ld) in place, cls_token | None, pos_spatial,
# pos_temporal | None (None: pos_spatial is the full table), pos_class | None
def expect_posenc(i, p):
    B, T, HW, Cc, ld = p["B"], p["T"], p["HW"], p["C"], p["ld"]
    x0 = i["x"].cpu()
    cls, ps, pt, pc = (None if i[k] is None else i[k].cpu() for k in ("cls_token", "pos_spatial", "pos_temporal", "pos_class"))
    has_cls = int(cls is not None)
    R = T * HW + has_cls
    # fp32: one or two fp32 adds in the kernel's order, x + (pos_spatial + pos_temporal), bit for bit; bf16: float64
    wide = torch.float32 if x0.dtype == torch.float32 else torch.float64
    x = rows_of(x0, B * R, ld, Cc).to(wide).reshape(B, R, Cc).clone()
    ps, pt, pc, clsw = (None if t is None else t.to(wide) for t in (ps, pt, pc, cls))
    if pt is not None:
        table = (ps[None, :, :] + pt[:, None, :]).reshape(T * HW, Cc)
        cls_row = None if cls is None else (clsw + pc if pc is not None else clsw)
    else:
        table = ps[has_cls:]
        cls_row = None if cls is None else clsw + ps[0]
    x[:, has_cls:] = x[:, has_cls:] + table
    if has_cls:
        x[:, 0] = cls_row
    owned = torch.ones(B, R, dtype=torch.bool)
    if p["cls_only"]:
        owned[:, 1:] = False
    tol = None if x0.dtype == torch.float32 else TOL[x0.dtype]
    return Expect(x.view(1, B * R, Cc), x0, ld, tol=tol, owned=owned.view(1, B * R))


def check_posenc(got, i, p):
    return expect_posenc(i, p).check(got, "pv_add_posenc")


# ---- pv_add_act: p = rows, C, lda, ldb, ldy, act; i = a, b, y0 (a itself when y aliases a)
def expect_add_act(i, p):
    a = rows_of(i["a"].cpu(), p["rows"], p["lda"], p["C"]).double()
    b = rows_of(i["b"].cpu(), p["rows"], p["ldb"], p["C"]).double()
    return Expect(ref_act(a + b, p["act"]), i["y0"], p["ldy"], tol=TOL[i["y0"].dtype])


def check_add_act(got, i, p):
    return expect_add_act(i, p).check(got, "pv_add_act")


# ---- pv_pool3d: p = B, T, H, W, C, k, s, p (pad), mode, n_prefix, ldx, ldy; i = x (B, x_bs), y0 (B, y_bs)
def pool_out_dims(p):
    return tuple((n + 2 * pd - k) // s + 1 for n, k, s, pd in zip((p["T"], p["H"], p["W"]), p["k"], p["s"], p["p"]))


def ref_pool(grid, k, s, pad, mode, drop=None):
    """MaxPool3d / AvgPool3d (count_include_pad) of a (B, T, H, W, C) float64 grid, one window tap at a time.
    drop = (b, to, ho, wo, (dt, dh, dw)): that tap is left out of that one window (a defect for the checks' own test)."""
    is_max = mode == L.POOL_MAX
    fill = float("-inf") if is_max else 0.0
    B, T, H, W, Cc = grid.shape
    xp = torch.full((B, T + 2 * pad[0], H + 2 * pad[1], W + 2 * pad[2], Cc), fill, dtype=torch.float64)
    xp[:, pad[0]:pad[0] + T, pad[1]:pad[1] + H, pad[2]:pad[2] + W] = grid
    To, Ho, Wo = ((n + 2 * pd - kk) // ss + 1 for n, kk, ss, pd in zip((T, H, W), k, s, pad))
    out = torch.full((B, To, Ho, Wo, Cc), fill, dtype=torch.float64)
    for dt in range(k[0]):
        for dh in range(k[1]):
            for dw in range(k[2]):
                tap = xp[:, dt:dt + (To - 1) * s[0] + 1:s[0], dh:dh + (Ho - 1) * s[1] + 1:s[1], dw:dw + (Wo - 1) * s[2] + 1:s[2]]
                if drop is not None and drop[4] == (dt, dh, dw):
                    tap = tap.clone()
                    tap[drop[0], drop[1], drop[2], drop[3]] = fill
                out = torch.maximum(out, tap) if is_max else out + tap
    return out if is_max else out / (k[0] * k[1] * k[2])


def expect_pool(i, p, drop=None):
    B, T, H, W, Cc, npre = p["B"], p["T"], p["H"], p["W"], p["C"], p["n_prefix"]
    x = rows_of(i["x"].cpu(), npre + T * H * W, p["ldx"], Cc).double()
    To, Ho, Wo = pool_out_dims(p)
    pooled = ref_pool(x[:, npre:].reshape(B, T, H, W, Cc), p["k"], p["s"], p["p"], p["mode"], drop)
    want = torch.cat([x[:, :npre], pooled.reshape(B, To * Ho * Wo, Cc)], 1)
    exact = torch.ones(B, want.shape[1], dtype=torch.bool)      # prefix rows are copies; a maximum does no arithmetic
    if p["mode"] != L.POOL_MAX:
        exact[:, npre:] = False
    return Expect(want, i["y0"], p["ldy"], tol=TOL[i["y0"].dtype], exact=exact)


def check_pool(got, i, p):
    return expect_pool(i, p).check(got, "pv_pool3d")


# ---- pv_layernorm: p = rows, C, ldx, ldy, eps, g_period; i = x (1, rows*ldx; fp32 when x_f32), gamma, beta
# ((max(g_period, 1), C) or None), y0
def ref_layernorm(x, gamma, beta, eps, period, wrong_row=None):
    """wrong_row = r: row r takes its gamma / beta from the neighbouring period (table row (r + 1) % period)."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    idx = torch.arange(x.shape[0]) % max(period, 1)
    if wrong_row is not None:
        idx[wrong_row] = (idx[wrong_row] + 1) % max(period, 1)
    if gamma is not None:
        y = y * gamma.double()[idx]
    if beta is not None:
        y = y + beta.double()[idx]
    return y


def expect_layernorm(i, p, wrong_row=None):
    x = rows_of(i["x"].cpu(), p["rows"], p["ldx"], p["C"])[0]
    g, b = (None if i[k] is None else i[k].cpu().view(max(p["g_period"], 1), p["C"]) for k in ("gamma", "beta"))
    want = ref_layernorm(x, g, b, p["eps"], p["g_period"], wrong_row)[None]
    return Expect(want, i["y0"], p["ldy"], tol=TOL[i["y0"].dtype])


def check_layernorm(got, i, p):
    return expect_layernorm(i, p).check(got, "pv_layernorm")


# ---- pv_affine_rows: p = rows, C, ldx, ldy, act, n_prefix, rows_per_batch; i = x, gamma, beta, y0 (x itself in place)
def expect_affine(i, p):
    x = rows_of(i["x"].cpu(), p["rows"], p["ldx"], p["C"])[0].double()
    v = x
    if i["gamma"] is not None:
        v = v * i["gamma"].cpu().double()
    if i["beta"] is not None:
        v = v + i["beta"].cpu().double()
    want = ref_act(v, p["act"])
    owned = torch.ones(1, p["rows"], dtype=torch.bool)
    exact = ~owned
    if p["rows_per_batch"] > 0 and p["n_prefix"] > 0:
        skip = (torch.arange(p["rows"]) % p["rows_per_batch"]) < p["n_prefix"]
        want[skip] = x[skip]                       # out of place the prefix rows are copied through
        exact[0, skip] = i["y0"].dtype == i["x"].dtype
        if p["inplace"]:
            owned[0, skip] = False                 # in place they are not touched at all
    return Expect(want[None], i["y0"], p["ldy"], tol=TOL[i["y0"].dtype], exact=exact, owned=owned)


def check_affine(got, i, p):
    return expect_affine(i, p).check(got, "pv_affine_rows")


# ---- pv_se_gate: p = B, C, c_p, cr, nblk, inv_count; i = psum (B, nblk, c_p), w1, b1, w2, b2, y0 (B, c_p)
def expect_se_gate(i, p):
    Cc = p["C"]
    mean = i["psum"].cpu().double().sum(1)[:, :Cc] * p["inv_count"]
    hid = (mean @ i["w1"].cpu().double().t() + i["b1"].cpu().double()).clamp_min(0)
    want = torch.sigmoid(hid @ i["w2"].cpu().double().t() + i["b2"].cpu().double())
    return Expect(want[:, None], i["y0"], p["c_p"], tol=1e-5, written=p["c_p"])


def check_se_gate(got, i, p):
    return expect_se_gate(i, p).check(got, "pv_se_gate")


# ---- pv_ingest_ncdhw: p = B, C, T, H, W, c_p, ld; i = src (B, C, src_T, H, W), t_index | None, ch_scale | None,
# ch_shift | None, y0 (B, bs)
def _layout_bound(src_dtype, dst_dtype, affine):
    """Keyword arguments of Expect for a layout change: exact where nothing rounds, one bf16 rounding where it narrows."""
    if affine:
        return dict(tol=TOL[torch.float32] if dst_dtype == torch.float32 else BF16_ROUND)
    if src_dtype == torch.float32 and dst_dtype == torch.bfloat16:
        return dict(per_elem=BF16_ROUND)
    return dict()


def expect_ingest(i, p):
    src = i["src"].cpu().double()
    if i["t_index"] is not None:
        src = src[:, :, i["t_index"].cpu().long()]
    if i["ch_scale"] is not None:
        src = src * i["ch_scale"].cpu().double().view(1, -1, 1, 1, 1)
        if i["ch_shift"] is not None:
            src = src + i["ch_shift"].cpu().double().view(1, -1, 1, 1, 1)
    want = src.permute(0, 2, 3, 4, 1).reshape(p["B"], p["T"] * p["H"] * p["W"], p["C"])
    return Expect(want, i["y0"], p["ld"], written=p["c_p"],
                  **_layout_bound(i["src"].dtype, i["y0"].dtype, i["ch_scale"] is not None))


def check_ingest(got, i, p):
    return expect_ingest(i, p).check(got, "pv_ingest_ncdhw")


# ---- pv_egress_ncdhw: p = B, C, T, H, W, c_p, ld; i = src (B, bs) NDHWC rows, y0 (1, B*C*T*H*W + tail) contiguous NCDHW
def expect_egress(i, p):
    S3 = p["T"] * p["H"] * p["W"]
    rows = rows_of(i["src"].cpu(), S3, p["ld"], p["C"]).double()
    want = rows.permute(0, 2, 1).reshape(1, p["B"] * p["C"] * S3, 1)
    return Expect(want, i["y0"], 1, written=1, **_layout_bound(i["src"].dtype, i["y0"].dtype, False))


def check_egress(got, i, p):
    return expect_egress(i, p).check(got, "pv_egress_ncdhw")


# ---- pv_ensemble_scores: p = N, C, ld, V, mode; i = logits (1, N*ld), video_index (N), accum0 (V, C), counts0 (V)
# got = (accum, counts)
def expect_ensemble(i, p):
    x = rows_of(i["logits"].cpu(), p["N"], p["ld"], p["C"])[0].double()
    acc, cnt = i["accum0"].cpu().double().clone(), i["counts0"].cpu().clone()
    seen = torch.zeros(p["V"], dtype=torch.bool)
    for n, v in enumerate(i["video_index"].cpu().tolist()):
        if v < 0 or v >= p["V"]:
            continue
        pr = torch.softmax(x[n], -1)
        acc[v] = torch.maximum(acc[v], pr) if p["mode"] == 1 else acc[v] + pr
        cnt[v] += 1
        seen[v] = True
    return Expect(acc[None], i["accum0"].cpu().view(1, -1), p["C"], tol=TOL[torch.float32], exact=~seen[None], written=p["C"]), cnt


def check_ensemble(got, i, p):
    e, cnt = expect_ensemble(i, p)
    err = e.check(got[0].view(1, -1), "pv_ensemble_scores")
    assert torch.equal(got[1].cpu(), cnt), "pv_ensemble_scores: counts %s, want %s" % (got[1].cpu().tolist(), cnt.tolist())
    return err


# ---- case builders (CPU tensors; the GPU tests move them to the device) ----------------------------------------------
def make_softmax(dtype, rows, Cc, inplace, seed=701):
    x = randn((1, rows, Cc), seed, 3.0).to(dtype).float()
    x[0, 0] = torch.where(torch.arange(Cc) % 2 == 0, 80.0, -80.0)      # the max subtraction matters
    if rows > 1:
        x[0, rows - 1] = 1.25                                           # a row of equal values
    ldx = round_up8(Cc) + 8
    ldy = ldx if inplace else ldx + 16
    xb = rows_buf(x, ldx, dtype)
    return dict(x=xb, y0=xb if inplace else canary_buf(1, rows * ldy, dtype)), dict(rows=rows, C=Cc, ldx=ldx, ldy=ldy)


def make_mean(dtype, B, rpb, Cc, seed=711):
    ldx, ldy = round_up8(Cc) + 8, round_up8(Cc) + 16
    x = rows_buf(randn((1, B * rpb, Cc), seed, 1.0, 0.5), ldx, dtype)
    return dict(x=x, y0=canary_buf(1, B * ldy, torch.float32)), dict(rows=B * rpb, rows_per_batch=rpb, C=Cc, ldx=ldx, ldy=ldy)


POSENC_FORMS = {          # form: (cls token, separable tables, pos_class)
    "sep_cls_posclass": (True, True, True), "sep_cls": (True, True, False), "sep_nocls": (False, True, False),
    "full_cls": (True, False, False), "full_nocls": (False, False, False),
}


def make_posenc(dtype, form, Cc, ld, cls_only=0, B=2, T=3, HW=5, seed=721):
    cls, sep, pc = POSENC_FORMS[form]
    R = T * HW + int(cls)
    x = rows_buf(randn((1, B * R, Cc), seed), ld, dtype)
    i = dict(x=x, cls_token=randn((Cc,), seed + 1) if cls else None,
             pos_spatial=randn((HW if sep else R, Cc), seed + 2), pos_temporal=randn((T, Cc), seed + 3) if sep else None,
             pos_class=randn((Cc,), seed + 4) if pc else None)
    return i, dict(B=B, T=T, HW=HW, C=Cc, ld=ld, cls_only=cls_only)


def make_add_act(dtype, rows, Cc, act, alias, seed=731):
    lda, ldb, ldy = round_up8(Cc) + 8, round_up8(Cc), round_up8(Cc) + 16
    if alias:
        ldy = lda
    a = rows_buf(randn((1, rows, Cc), seed, 2.0), lda, dtype)
    b = rows_buf(randn((1, rows, Cc), seed + 1, 2.0), ldb, dtype)
    return dict(a=a, b=b, y0=a if alias else canary_buf(1, rows * ldy, dtype)), dict(rows=rows, C=Cc, lda=lda, ldb=ldb, ldy=ldy, act=act)


def make_pool(dtype, B, T, H, W, Cc, k, s, pad, mode, n_prefix=0, gap=0, seed=741):
    p = dict(B=B, T=T, H=H, W=W, C=Cc, k=tuple(k), s=tuple(s), p=tuple(pad), mode=mode, n_prefix=n_prefix)
    cp = round_up8(Cc)
    p["ldx"], p["ldy"] = cp + (8 if gap else 0), cp + (16 if gap else 0)
    To, Ho, Wo = pool_out_dims(p)
    Rx, Ry = n_prefix + T * H * W, n_prefix + To * Ho * Wo
    p["x_bs"], p["y_bs"] = Rx * p["ldx"] + gap, Ry * p["ldy"] + 2 * gap
    x = rows_buf(randn((B, Rx, Cc), seed), p["ldx"], dtype, bs=p["x_bs"])
    return dict(x=x, y0=canary_buf(B, p["y_bs"], dtype)), p


def make_layernorm(dtype, rows, Cc, x_f32=False, g_period=0, gamma=True, beta=True, ramp=False, seed=751):
    ldx, ldy = round_up8(Cc) + 8, round_up8(Cc) + 16
    x = rows_buf(randn((1, rows, Cc), seed, 2.0, 0.5), ldx, torch.float32 if x_f32 else dtype)
    P = max(g_period, 1)
    g = randn((P, Cc), seed + 1, 0.3, 1.0) if gamma else None
    if ramp:                                  # table rows a wrong period cannot be mistaken for: gamma row i = 1 + i
        g = (1.0 + torch.arange(P, dtype=torch.float32))[:, None].repeat(1, Cc)
    b = randn((P, Cc), seed + 2, 0.5) if beta else None
    return (dict(x=x, gamma=g, beta=b, y0=canary_buf(1, rows * ldy, dtype)),
            dict(rows=rows, C=Cc, ldx=ldx, ldy=ldy, eps=1e-6, g_period=g_period, x_f32=int(x_f32)))


def make_affine(dtype, rows, Cc, x_f32, inplace, act, n_prefix=0, rpb=0, seed=761):
    ldx = round_up8(Cc) + 8
    ldy = ldx if inplace else ldx + 8
    x = rows_buf(randn((1, rows, Cc), seed), ldx, torch.float32 if x_f32 else dtype)
    g, b = randn((Cc,), seed + 1, 0.3, 1.0), randn((Cc,), seed + 2, 0.4)
    return (dict(x=x, gamma=g, beta=b, y0=x if inplace else canary_buf(1, rows * ldy, dtype)),
            dict(rows=rows, C=Cc, ldx=ldx, ldy=ldy, act=act, n_prefix=n_prefix, rows_per_batch=rpb, x_f32=int(x_f32), inplace=inplace))


def make_se_gate(B, Cc, cr, nblk, extra_pad=0, seed=771):
    cp = round_up8(Cc) + extra_pad
    psum = torch.zeros(B, nblk, cp)
    psum[..., :Cc] = randn((B, nblk, Cc), seed, 3.0)
    i = dict(psum=psum, w1=randn((cr, Cc), seed + 1, Cc ** -0.5), b1=randn((cr,), seed + 2),
             w2=randn((Cc, cr), seed + 3, cr ** -0.5), b2=randn((Cc,), seed + 4), y0=canary_buf(B, cp, torch.float32))
    return i, dict(B=B, C=Cc, c_p=cp, cr=cr, nblk=nblk, inv_count=1.0 / 777.0)


def _src_values(shape, dtype, seed):
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return randn(shape, seed, 2.0).to(dtype)


def make_ingest(src_dtype, dst_dtype, Cc, H, W, c_p, ld, affine, shift=True, misalign=False, B=2, T=3, src_T=5, gap=16, seed=781):
    """affine: frame selection (t_index) and the per-channel map ride along, as the data pipeline uses them."""
    Ts = src_T if affine else T
    n = B * Cc * Ts * H * W
    flat = _src_values((n + 1,), src_dtype, seed)
    src = (flat[1:] if misalign else flat[:n]).view(B, Cc, Ts, H, W)      # misalign: one element past the allocation's start
    bs = T * H * W * ld + gap
    i = dict(src=src, t_index=None, ch_scale=None, ch_shift=None, y0=canary_buf(B, bs, dst_dtype))
    if affine:
        i["t_index"] = torch.tensor([4, 0, 2], dtype=torch.int32)[:T]
        i["ch_scale"] = randn((Cc,), seed + 1, 0.1, 1.0) / (255.0 if src_dtype == torch.uint8 else 1.0)
        i["ch_shift"] = randn((Cc,), seed + 2, 0.5) if shift else None
    return i, dict(B=B, C=Cc, T=T, H=H, W=W, c_p=c_p, ld=ld, bs=bs, src_T=Ts)


def make_egress(src_dtype, dst_dtype, Cc=11, c_p=16, ld=24, B=2, T=3, H=5, W=7, gap=16, seed=791):
    S3 = T * H * W
    bs = S3 * ld + gap
    src = rows_buf(randn((B, S3, Cc), seed, 2.0), ld, src_dtype, bs=bs, written=c_p)
    return dict(src=src, y0=canary_buf(1, B * Cc * S3 + 16, dst_dtype)), dict(B=B, C=Cc, T=T, H=H, W=W, c_p=c_p, ld=ld, bs=bs)


def make_ensemble(mode, seed=801):
    N, Cc, V = 11, 13, 4
    ld = Cc + 8
    idx = torch.tensor([0, 1, 2, 0, -1, 1, 2, V, 0, 1, 2], dtype=torch.int32)     # video 3 gets no clip; -1 and V are ignored
    logits = rows_buf(randn((1, N, Cc), seed, 3.0), ld, torch.float32, written=Cc)
    accum0 = torch.rand((V, Cc), generator=torch.Generator().manual_seed(seed + 1)) * (0.2 if mode == 1 else 1.0)
    return (dict(logits=logits, video_index=idx, accum0=accum0, counts0=torch.tensor([3, 0, 5, 2], dtype=torch.int32)),
            dict(N=N, C=Cc, ld=ld, V=V, mode=mode))


# ------------------------------------------------------------------ stencil family (pv_dwconv.hip, pv_pwdw.hip, pv_tokpool.hip)
# float64 references and checks of pv_dwconv3d (depthwise / grouped, psum, cls prefix, w_mod, fused pointwise producer) and
# pv_token_pool.  tests/test_stencil_kernel_checks.py feeds the checks their own reference and defective copies of it;
# tests/test_gpu_stencil_kernels.py feeds them what the kernels left on the device.
PSUM_TOL, PSUM_TOL_FUSED = 1e-3, 2e-3      # mean over T,H,W taken from psum (tests/test_gpu_kernels.py)


def round_up32(c):
    return (c + 31) // 32 * 32


def conv_out_dims(p):
    return tuple((n + 2 * pd - k) // s + 1 for n, k, s, pd in zip((p["T"], p["H"], p["W"]), p["k"], p["s"], p["p"]))


def ref_stencil(grid, w, s, pad, gw=1, halo=None, drop=None):
    """nn.Conv3d(C, C, k, s, pad, groups=C // gw, bias=False) of a (B, T, H, W, C) float64 grid; w (C, gw, kt, kh, kw).
    halo: (C,) value the padding is filled with instead of zero; drop = (b, to, ho, wo, (dt, dh, dw)): that tap is left out
    of that one output voxel (both are defects for the checks' own test)."""
    import torch.nn.functional as F
    B, T, H, W, Cc = grid.shape
    xp = torch.zeros(B, T + 2 * pad[0], H + 2 * pad[1], W + 2 * pad[2], Cc, dtype=torch.float64)
    if halo is not None:
        xp[:] = halo.double()
    xp[:, pad[0]:pad[0] + T, pad[1]:pad[1] + H, pad[2]:pad[2] + W] = grid
    out = F.conv3d(xp.permute(0, 4, 1, 2, 3), w.double(), None, stride=s, padding=0, groups=Cc // gw).permute(0, 2, 3, 4, 1).contiguous()
    if drop is not None:
        assert gw == 1
        b, to, ho, wo, (dt, dh, dw) = drop
        out[b, to, ho, wo] -= xp[b, to * s[0] + dt, ho * s[1] + dh, wo * s[2] + dw] * w.double()[:, 0, dt, dh, dw]
    return out


def pack_dw_weights(w, w_p):
    """(Cw, gw, kt, kh, kw) -> the library's [taps][gw][w_p] fp32 block, zero padded."""
    Cw, gw = w.shape[:2]
    taps = w[0, 0].numel()
    wp = torch.zeros(taps, gw, w_p, dtype=torch.float32)
    wp[:, :, :Cw] = w.reshape(Cw, gw, taps).permute(2, 1, 0)
    return wp


def fill_dw_geometry(d, p, dtype):
    """Every field of a DwConv3dDesc that is not a pointer."""
    To, Ho, Wo = conv_out_dims(p)
    d.x_bs, d.y_bs, d.ldx, d.ldy = p["x_bs"], p["y_bs"], p["ldx"], p["ldy"]
    d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = p["B"], p["T"], p["H"], p["W"], p["C"], To, Ho, Wo
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*p["k"], *p["s"], *p["p"])
    d.w_mod, d.act, d.n_prefix, d.gw = p["w_mod"], p["act"], p["n_prefix"], p["gw"]
    d.dtype = L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32
    d.pw_cin, d.pw_act = p.get("pw_cin", 0), p.get("pw_act", 0)
    return d


# ---- pv_dwconv3d: p = B, T, H, W, C, k, s, p (pad), act, gw, w_mod, n_prefix, ldx, ldy, x_bs, y_bs, x_off, psum;
# i = x (B, x_bs; the grid's channels start at column x_off of every row), y0 (B, y_bs), w (packed), wref (Cw, gw, kt, kh, kw),
# scale, shift (C,)
def _x_rows(i, p, R, Cc):
    buf = i["x"].cpu()
    return buf[:, :R * p["ldx"]].view(buf.shape[0], R, p["ldx"])[..., p.get("x_off", 0):p.get("x_off", 0) + Cc]


def expect_dwconv(i, p, drop=None, wrong_head=False, prefix_from=0):
    """(Expect for y, pre-activation reference (B, To*Ho*Wo, C)).  wrong_head: the channels of every head but the first take
    the shared filter one 8-channel chunk over (a lane that reduces its chunk modulo the wrong width); prefix_from = 1: the
    prefix rows are copied from one row further down."""
    B, T, H, W, Cc, npre, gw = p["B"], p["T"], p["H"], p["W"], p["C"], p["n_prefix"], max(p["gw"], 1)
    rows = _x_rows(i, p, npre + T * H * W, Cc).double()
    w = i["wref"].double()
    if p["w_mod"] > 0:
        idx = torch.arange(Cc) % p["w_mod"]
        if wrong_head:
            idx = torch.where(torch.arange(Cc) >= p["w_mod"], (idx + 8) % p["w_mod"], idx)
        w = w[idx]
    pre = ref_stencil(rows[:, npre:].reshape(B, T, H, W, Cc), w, p["s"], p["p"], gw, drop=drop)
    pre = pre * i["scale"].double() + i["shift"].double()
    pre = pre.reshape(B, -1, Cc)
    want = torch.cat([rows[:, prefix_from:prefix_from + npre], ref_act(pre, p["act"])], 1)
    exact = torch.zeros(B, want.shape[1], dtype=torch.bool)
    exact[:, :npre] = True                                     # cls rows are copies
    return Expect(want, i["y0"], p["ldy"], tol=TOL[i["y0"].dtype], exact=exact), pre


def check_psum(psum, pre, p, nblk, tol, what="pv_dwconv3d"):
    """psum (B * nblk + 1, round_up(C, 8)) as the launch left it (NaN before): every entry of the B * nblk blocks finite, the
    padding channels exactly zero, the one block behind them untouched, and the mean over T,H,W within tol of the reference's."""
    psum, Cc, B = psum.detach().cpu(), p["C"], p["B"]
    assert psum.shape == (B * nblk + 1, round_up8(Cc)), what
    body = psum[:B * nblk].view(B, nblk, -1)
    assert torch.isfinite(body).all(), "%s: %d psum entries were not written" % (what, (~torch.isfinite(body)).sum().item())
    assert (body[..., Cc:] == 0).all(), "%s: padding channels of psum are not zero" % what
    assert torch.isnan(psum[-1]).all(), "%s: the psum block behind the last one was written" % what
    err = _abs_rel(body[..., :Cc].double().sum(1) / pre.shape[1], pre.mean(1))
    assert err <= tol, "%s: mean from psum off by %.3e of the reference abs-max > %.1e" % (what, err, tol)
    return err


def check_dwconv(got, i, p, psum=None, nblk=0):
    """-> (error of y, error of the psum mean or None)"""
    e, pre = expect_pwdw(i, p) if p.get("pw_cin", 0) else expect_dwconv(i, p)
    what = "pv_dwconv3d(pw)" if p.get("pw_cin", 0) else "pv_dwconv3d"
    err = e.check(got, what)
    if psum is None:
        return err, None
    return err, check_psum(psum, pre, p, nblk, PSUM_TOL_FUSED if p.get("pw_cin", 0) else PSUM_TOL, what)


def make_dwconv(dtype, B, T, H, W, Cc, k, s, pad, act, gw=0, w_mod=0, n_prefix=0, ldx=None, ldy=None, gap=16, qkv=False, seed=901):
    """qkv: x is the middle third of a fused (q | k | v) token buffer, ldx = 3 * C."""
    p = dict(B=B, T=T, H=H, W=W, C=Cc, k=tuple(k), s=tuple(s), p=tuple(pad), act=act, gw=gw, w_mod=w_mod, n_prefix=n_prefix)
    cp = round_up8(Cc)
    To, Ho, Wo = conv_out_dims(p)
    Rx, Ry = n_prefix + T * H * W, n_prefix + To * Ho * Wo
    p["ldx"], p["ldy"] = (3 * Cc if qkv else cp) if ldx is None else ldx, cp if ldy is None else ldy
    p["x_bs"], p["y_bs"], p["x_off"] = Rx * p["ldx"] + gap, Ry * p["ldy"] + 2 * gap, Cc if qkv else 0
    if qkv:
        assert Cc % 8 == 0
        x = torch.full((B, p["x_bs"]), CANARY, dtype=dtype)
        x[:, :Rx * p["ldx"]] = randn((B, Rx * p["ldx"]), seed).to(dtype)
    else:
        x = rows_buf(randn((B, Rx, Cc), seed), p["ldx"], dtype, bs=p["x_bs"])
    Cw, g = w_mod or Cc, max(gw, 1)
    wref = randn((Cw, g) + tuple(k), seed + 1, (g * k[0] * k[1] * k[2]) ** -0.5 * 1.7)
    i = dict(x=x, y0=canary_buf(B, p["y_bs"], dtype), w=pack_dw_weights(wref, round_up8(Cw)), wref=wref,
             scale=randn((Cc,), seed + 2, 0.2, 1.0), shift=randn((Cc,), seed + 3, 0.5, 0.25))
    return i, p


# ---- pv_dwconv3d with the fused pointwise producer: p as above + pw_cin, pw_act; i as above + x of pw_cin channels,
# pw_w (round_up(C, 32), round_up(pw_cin, 32)) bf16 zero padded, wa (C, pw_cin) bf16, pw_scale, pw_shift (C,)
def expect_pwdw(i, p, halo_shift=False, drop=None):
    """conv_a + affine + activation in float64, rounded to bf16, then the depthwise conv in float64; the expanded tensor is
    ZERO outside the image.  halo_shift: it is act(pw_shift) there instead (a defect: the image of a zero input)."""
    B, T, H, W, Cc, cin = p["B"], p["T"], p["H"], p["W"], p["C"], p["pw_cin"]
    x = _x_rows(i, p, T * H * W, cin).double()
    h = ref_act((x @ i["wa"].double().t()) * i["pw_scale"].double() + i["pw_shift"].double(), p["pw_act"])
    h = h.to(torch.bfloat16).double().reshape(B, T, H, W, Cc)
    halo = ref_act(i["pw_shift"].double(), p["pw_act"]).to(torch.bfloat16).double() if halo_shift else None
    pre = ref_stencil(h, i["wref"].double(), p["s"], p["p"], 1, halo=halo, drop=drop)
    pre = (pre * i["scale"].double() + i["shift"].double()).reshape(B, -1, Cc)
    return Expect(ref_act(pre, p["act"]), i["y0"], p["ldy"], tol=TOL[torch.bfloat16]), pre


def make_pwdw(B, T, H, W, cin, Cc, stride, act, pw_act, wide_ldx=False, gap=16, seed=921):
    p = dict(B=B, T=T, H=H, W=W, C=Cc, k=(3, 3, 3), s=(1, stride, stride), p=(1, 1, 1), act=act, gw=0, w_mod=0, n_prefix=0,
             pw_cin=cin, pw_act=pw_act, x_off=0)
    cp, To, Ho, Wo = round_up8(Cc), *conv_out_dims(p)
    p["ldx"], p["ldy"] = round_up8(cin) + (16 if wide_ldx else 0), cp + 8
    p["x_bs"], p["y_bs"] = T * H * W * p["ldx"] + gap, To * Ho * Wo * p["ldy"] + 2 * gap
    wa = randn((Cc, cin), seed + 4, cin ** -0.5).to(torch.bfloat16)
    pw_w = torch.zeros(round_up32(Cc), round_up32(cin), dtype=torch.bfloat16)
    pw_w[:Cc, :cin] = wa
    wref = randn((Cc, 1, 3, 3, 3), seed + 1, 0.3)
    i = dict(x=rows_buf(randn((B, T * H * W, cin), seed), p["ldx"], torch.bfloat16, bs=p["x_bs"]),
             y0=canary_buf(B, p["y_bs"], torch.bfloat16), w=pack_dw_weights(wref, cp), wref=wref,
             scale=randn((Cc,), seed + 2, 0.2, 1.0), shift=randn((Cc,), seed + 3, 0.5, 0.25),
             pw_w=pw_w, wa=wa, pw_scale=randn((Cc,), seed + 5, 0.2, 1.0), pw_shift=randn((Cc,), seed + 6, 0.5, 0.3))
    return i, p


# ---- pv_token_pool: p = n, B, T, H, W, heads, hd, k, strides [n], n_prefix, eps, ldx [n], ldy [n], x_bs [n], y_bs [n];
# i = x [n] (B, x_bs), y0 [n] (B, y_bs), w [n] ([taps][hd] packed), wref [n] (hd, 1, kt, kh, kw), gamma [n], beta [n] ((hd,) | None)
def token_pool_out_dims(p, z):
    return tuple((n + 2 * (k // 2) - k) // s + 1 for n, k, s in zip((p["T"], p["H"], p["W"]), p["k"], p["strides"][z]))


def expect_token_pool(i, p, z, stat_width=None, drop=None, prefix_from=0):
    """Tensor z of the launch.  stat_width: the LayerNorm statistics are taken over that many channels (the head's, then
    zeros) instead of head_dim -- a defect for the checks' own test."""
    B, T, H, W, heads, hd, npre = p["B"], p["T"], p["H"], p["W"], p["heads"], p["hd"], p["n_prefix"]
    Cw = heads * hd
    rows = rows_of(i["x"][z].cpu(), npre + T * H * W, p["ldx"][z], Cw).double()
    To, Ho, Wo = token_pool_out_dims(p, z)
    grid = rows[:, npre:].reshape(B, T, H, W, Cw)
    w = i["wref"][z].double()[torch.arange(Cw) % hd]
    pooled = ref_stencil(grid, w, p["strides"][z], tuple(kk // 2 for kk in p["k"]), 1, drop=drop)[:, :To, :Ho, :Wo]
    v = torch.cat([rows[:, prefix_from:prefix_from + npre], pooled.reshape(B, -1, Cw)], 1).reshape(B, -1, heads, hd)
    g, bt = i["gamma"][z], i["beta"][z]
    if g is not None or bt is not None:
        n = stat_width or hd
        mean = v.sum(-1, keepdim=True) / n
        var = (((v - mean) ** 2).sum(-1, keepdim=True) + (n - hd) * mean ** 2) / n
        v = (v - mean) / torch.sqrt(var + p["eps"])
        if g is not None:
            v = v * g.double()
        if bt is not None:
            v = v + bt.double()
    exact = None
    if g is None and bt is None and npre:                      # nothing is computed on a cls row that is not normalised
        exact = torch.zeros(B, v.shape[1], dtype=torch.bool)
        exact[:, :npre] = True
    return Expect(v.reshape(B, -1, Cw), i["y0"][z], p["ldy"][z], tol=TOL[i["y0"][z].dtype], exact=exact, written=Cw)


def check_token_pool(gots, i, p):
    return max(expect_token_pool(i, p, z).check(gots[z], "pv_token_pool[%d]" % z) for z in range(p["n"]))


def make_token_pool(dtype, B, heads, hd, thw, k, strides, n_prefix, gamma=True, beta=True, wide=False, gap=0, seed=941):
    T, H, W = thw
    n, Cw = len(strides), heads * hd
    p = dict(n=n, B=B, T=T, H=H, W=W, heads=heads, hd=hd, k=tuple(k), strides=[tuple(s) for s in strides], n_prefix=n_prefix,
             eps=1e-6, ldx=[], ldy=[], x_bs=[], y_bs=[])
    i = dict(x=[], y0=[], w=[], wref=[], gamma=[], beta=[])
    for z in range(n):
        To, Ho, Wo = token_pool_out_dims(p, z)
        Rx, Ry = n_prefix + T * H * W, n_prefix + To * Ho * Wo
        ldx, ldy = Cw + (8 if wide else 0), Cw + (16 if wide else 0)
        p["ldx"].append(ldx), p["ldy"].append(ldy), p["x_bs"].append(Rx * ldx + gap), p["y_bs"].append(Ry * ldy + 2 * gap)
        wref = randn((hd, 1) + tuple(k), seed + 10 * z + 1, (k[0] * k[1] * k[2]) ** -0.5 * 1.7)
        i["x"].append(rows_buf(randn((B, Rx, Cw), seed + 10 * z, 1.0, 0.3), ldx, dtype, bs=p["x_bs"][z], written=Cw))
        i["y0"].append(canary_buf(B, p["y_bs"][z], dtype))
        i["w"].append(pack_dw_weights(wref, hd).reshape(-1, hd)), i["wref"].append(wref)
        i["gamma"].append(randn((hd,), seed + 10 * z + 2, 0.2, 1.0) if gamma else None)
        i["beta"].append(randn((hd,), seed + 10 * z + 3, 0.3) if beta else None)
    return i, p


# ------------------------------------------------------------------ streaming conv family (pv_pwconv.hip, pv_lateral.hip, pv_stem.hip)
# pw_stream_kernel, tap_stream_kernel and stem_c4_kernel launch about one resident generation of workgroups and walk the voxel
# groups in a grid-stride loop.  The float64 references and the two checks below serve tests/test_gpu_stream_kernels.py, whose
# cases run several trips of that loop; tests/test_stream_kernel_checks.py feeds the checks their own reference and defective
# copies of it on the CPU.
#
# An output is ONE allocation: STREAM_GUARD canaries, M rows of `ld` elements, STREAM_GUARD canaries.  A launch owns channels
# [c_off, c_off + round_up(cout, 8)) of every row; the rest of a row (the slow pathway's slice of a lateral connection) comes
# back as it went in.
STREAM_GUARD = 4096


def cdiv(a, b):
    return -(-a // b)


def stream_chunks(resident, per_cu, nsplit):
    """Candidate `nchunks` of a launcher that sizes its grid as ceil(resident * per_cu / nsplit), for every residency the
    runtime may report."""
    return [cdiv(resident * p, nsplit) for p in per_cu]


def assert_trips(ngroups, candidates, full=2):
    """The condition on the INPUTS of a multi-trip case: under every candidate grid the loop runs more than `full` whole trips'
    worth of groups and the last trip is ragged (some workgroups run one trip more than their neighbours)."""
    for n in candidates:
        assert ngroups > full * n, "ngroups %d is no more than %d trips of %d chunks" % (ngroups, full, n)
        assert ngroups % n != 0, "ngroups %d is a whole number of trips of %d chunks" % (ngroups, n)


def stream_buf(M, ld, dtype, fill=None, guard=STREAM_GUARD):
    """The allocation of an output: canaries everywhere, or rows of `fill` (M, ld) between the two guards."""
    buf = torch.full((2 * guard + M * ld,), CANARY, dtype=dtype)
    if fill is not None:
        buf[guard:guard + M * ld] = fill.reshape(-1).to(dtype)
    return buf


class StreamExpect:
    """What one launch of a streaming conv kernel must leave in its output allocation.

    want     (M, cout) float64 reference
    before   the allocation as it was handed to the launch (stream_buf)
    S        voxels per clip; gvox: voxels (MFMA columns) per group of the grid-stride loop
    nchunks  candidate grid sizes in chunks; a failure names g // n for each, the trip of the loop the voxel was computed on
    unit     (M,) index of the MFMA column a voxel sits in, where that is not the voxel itself (two outputs per column)
    """

    def __init__(self, want, before, ld, S, gvox, nchunks, tol, c_off=0, unit=None, guard=STREAM_GUARD):
        self.want, self.before, self.ld, self.S, self.gvox = want.cpu().double(), before.cpu().clone(), ld, S, gvox
        self.nchunks, self.tol, self.c_off, self.unit, self.guard = list(nchunks), tol, c_off, unit, guard
        self.M, self.C = want.shape
        self.written = round_up8(self.C)
        assert self.before.numel() == 2 * guard + self.M * ld and c_off + self.written <= ld

    def rows(self, buf):
        return buf[self.guard:self.guard + self.M * self.ld].view(self.M, self.ld)

    def group_of(self, m):
        return int(m if self.unit is None else self.unit[m]) // self.gvox

    def where(self, m, c=None):
        """Place of voxel m in the loop (c, the output channel, places nothing here: a group spans every channel of its split)."""
        g = self.group_of(m)
        return "voxel %d (clip %d, voxel %d of it), group g = %d, trip g // nchunks = %s" % (
            m, m // self.S, m % self.S, g, ", ".join("%d of nchunks %d" % (g // n, n) for n in self.nchunks))

    def ideal(self):
        """The allocation a kernel that computes the reference exactly leaves."""
        buf = self.before.clone()
        r = self.rows(buf)
        r[:, self.c_off:self.c_off + self.C] = self.want.to(buf.dtype)
        r[:, self.c_off + self.C:self.c_off + self.written] = 0
        return buf

    def check(self, got, what=""):
        """-> error relative to the reference abs-max.  The message of a failure carries the worst voxel's place in the loop."""
        got = got.detach().cpu()
        assert got.shape == self.before.shape and got.dtype == self.before.dtype, what
        g, n = self.guard, self.M * self.ld
        bad = (got[:g] != self.before[:g]).sum().item() + (got[g + n:] != self.before[g + n:]).sum().item()
        assert bad == 0, "%s: %d canary elements around the output changed" % (what, bad)
        r = self.rows(got)
        diff = (r[:, self.c_off:self.c_off + self.C].double() - self.want).abs()
        diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
        per_voxel = diff.max(1).values
        m = int(per_voxel.argmax())
        err = per_voxel[m].item() / max(self.want.abs().max().item(), 1e-6)
        assert err <= self.tol, "%s: error %.3e of the reference abs-max > %.1e, worst at %s, channel %d" % (
            what, err, self.tol, self.where(m, int(diff[m].argmax())), int(diff[m].argmax()))
        pads = r[:, self.c_off + self.C:self.c_off + self.written]
        if pads.numel() and (pads != 0).any():
            m = int((pads != 0).any(1).nonzero()[0])
            raise AssertionError("%s: %d padding channels are not zero, first at %s" % (
                what, (pads != 0).sum().item(), self.where(m, self.C + int((pads[m] != 0).nonzero()[0]))))
        rest_got, rest_before = r.clone(), self.rows(self.before).clone()
        rest_got[:, self.c_off:self.c_off + self.written] = 0
        rest_before[:, self.c_off:self.c_off + self.written] = 0
        bad = (rest_got != rest_before).sum().item()
        assert bad == 0, "%s: %d elements of the rows that the launch does not own changed" % (what, bad)
        return err

    def check_trips(self, got, pieces, what=""):
        """Trip invariance, bit for bit: `pieces` is an allocation like `got` that a series of one-trip sub-launches filled
        (each through a pointer offset into it).  A voxel's value comes from the same instruction sequence in the same order on
        any trip of the loop and in any MFMA column, so the two allocations are equal; nothing here is a tolerance."""
        got, pieces = got.detach().cpu(), pieces.detach().cpu()
        assert got.shape == pieces.shape == self.before.shape and got.dtype == pieces.dtype, what
        if torch.equal(got, pieces):
            return
        g, n = self.guard, self.M * self.ld
        assert torch.equal(got[:g], pieces[:g]) and torch.equal(got[g + n:], pieces[g + n:]), "%s: the canaries differ" % what
        ne = self.rows(got) != self.rows(pieces)
        voxels = ne.any(1).nonzero().flatten()
        m = int(voxels[0])
        c = int(ne[m].nonzero()[0])
        raise AssertionError("%s: the large launch and the one-trip sub-launches differ in %d elements of %d voxels; first at %s, "
                             "column %d of the row: %r against %r; last at %s" % (
                                 what, ne.sum().item(), len(voxels), self.where(m, c - self.c_off), c, self.rows(got)[m, c].item(),
                                 self.rows(pieces)[m, c].item(),
                                 self.where(int(voxels[-1]), int(ne[int(voxels[-1])].nonzero()[-1]) - self.c_off)))


def ref_pointwise(x, w, scale, shift, act, gate=None, a_act=0, clip=None, res=None, x2=None, w2=None, scale2=None):
    """pw_stream_kernel's operation in float64: act(((a(x * gate[clip])) @ w^T) * scale + shift + (x2 @ w2^T) * scale2 + res).
    x (M, cin), w (cout, cin), gate (B, cin), clip (M,) the clip whose gate row a voxel takes, res (M, cout), x2 (M, cin2) the
    second operand already gathered.  The gated / activated operand is rounded to bf16 where the kernel rounds it."""
    xin = x.double()
    if gate is not None:
        xin = xin * gate.double()[clip]
    if gate is not None or a_act:
        xin = ref_act(xin, a_act).to(torch.bfloat16).double()
    out = (xin @ w.double().t()) * scale.double() + shift.double()
    if x2 is not None:
        out = out + (x2.double() @ w2.double().t()) * scale2.double()
    if res is not None:
        out = out + res.double()
    return ref_act(out, act)


def ref_tap_conv(x, w, stride, pad, scale=None, shift=None, act=0):
    """nn.Conv3d(cin, cout, k, stride, pad, bias=False) + affine + activation of a (B, T, H, W, cin) grid in float64, one filter
    tap at a time; w (cout, cin, kt, kh, kw).  -> (B, To, Ho, Wo, cout)"""
    B, T, H, W, cin = x.shape
    cout, _, kt, kh, kw = w.shape
    xp = torch.zeros(B, T + 2 * pad[0], H + 2 * pad[1], W + 2 * pad[2], cin, dtype=torch.float64, device=x.device)
    xp[:, pad[0]:pad[0] + T, pad[1]:pad[1] + H, pad[2]:pad[2] + W] = x
    To, Ho, Wo = ((n + 2 * p - k) // s + 1 for n, p, k, s in zip((T, H, W), pad, (kt, kh, kw), stride))
    out = torch.zeros(B * To * Ho * Wo, cout, dtype=torch.float64, device=x.device)
    wd = w.double()
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                tap = xp[:, dt:dt + (To - 1) * stride[0] + 1:stride[0], dh:dh + (Ho - 1) * stride[1] + 1:stride[1],
                         dw:dw + (Wo - 1) * stride[2] + 1:stride[2]]
                out.addmm_(tap.reshape(-1, cin), wd[:, :, dt, dh, dw].t())
    if scale is not None:
        out = out * scale.double()
    if shift is not None:
        out = out + shift.double()
    return ref_act(out, act).view(B, To, Ho, Wo, cout)


def ref_tap_pw2(x, w, stride, pad, scale, shift, act, w2, scale2, shift2, act2, res=None):
    """tap_stream_kernel's two-conv form: the inner tensor is rounded to bf16 (it becomes an MFMA operand), then the pointwise
    conv, its affine, the residual and its activation in float64.  -> (M, cout2)"""
    mid = ref_tap_conv(x, w, stride, pad, scale, shift, act).to(torch.bfloat16).double()
    return ref_pointwise(mid.reshape(-1, mid.shape[-1]), w2, scale2, shift2, act2, res=res)


# ------------------------------------------------------------------ dense GEMM family (pv_gemm.hip, pv_gemm8.hip, pv_gemm9.hip, pv_gemm9h.hip)
# gemm_glds_kernel, gemm8_kernel, gemm_quad_kernel and gemm_quad_half_kernel are persistent: the launcher starts
# min(total_tiles, R) workgroups (R = 512 for gemm_glds_kernel, 256 for the others) and workgroup w walks the work items
# it = w, w + R, w + 2 R, ... of the XCD-aware tile order of pv_gemm_tile.h.  The mirror of that order and GemmExpect serve
# tests/test_gpu_gemm_kernels.py, whose cases run more than two trips of that loop; tests/test_gemm_kernel_checks.py feeds the
# checks their own reference and defective copies of it on the CPU.  The float64 references are ref_pointwise and ref_tap_conv.
def gemm_tile_of(it, total_tiles):
    """PvTileOrder (pv_gemm_tile.h): work item -> tile.  Works on ints and on integer arrays / tensors alike."""
    xcd, slot = it & 7, it >> 3
    qn, rn = total_tiles >> 3, total_tiles & 7
    lo, hi = xcd * (qn + 1), rn * (qn + 1) + (xcd - rn) * qn
    return (xcd < rn) * lo + (xcd >= rn) * hi + slot


def gemm_origin_of(it, total_tiles, tiles_n, BM, BN):
    """work item -> (m0, n0), the first voxel row and the first channel of its BM x BN tile"""
    tile = gemm_tile_of(it, total_tiles)
    return (tile // tiles_n) * BM, (tile % tiles_n) * BN


def gemm_item_of(tile, total_tiles):
    """The inverse of gemm_tile_of: tile -> work item.  XCD x owns the tiles [start(x), start(x) + qn + (x < rn))."""
    qn, rn = total_tiles >> 3, total_tiles & 7
    big = rn * (qn + 1)                                   # tiles of the XCDs that own one more
    if tile < big:
        xcd, slot = tile // (qn + 1), tile % (qn + 1)
    else:
        xcd, slot = rn + (tile - big) // qn, (tile - big) % qn
    return slot * 8 + xcd


def gemm_place(m, c, total_tiles, tiles_n, BM, BN, R):
    """(voxel row, channel) -> dict(tile, m0, n0, item, workgroup, trip) under a grid of R workgroups"""
    tile = (m // BM) * tiles_n + c // BN
    it = gemm_item_of(tile, total_tiles)
    grid = min(total_tiles, R)
    return dict(tile=tile, m0=m // BM * BM, n0=c // BN * BN, item=it, workgroup=it % grid, trip=it // grid)


def gemm_trip_conditions(M, S, cout, BM, BN, R, rotation=False):
    """The conditions on the INPUTS of a multi-trip GEMM case, asserted before anything is launched -> (tiles_m, tiles_n, total).
    More than two whole trips, a ragged last one, a remainder branch in the XCD order (total % 8 != 0), an M tail, and tiles
    that straddle clips.  A rotation case cannot have the last two: the launchers rotate only where a frame is a whole number
    of tiles (Ho Wo % BM == 0), so a clip and M are whole numbers of tiles as well; it asserts exactly that instead."""
    tiles_m, tiles_n = cdiv(M, BM), cdiv(round_up8(cout), BN)
    total = tiles_m * tiles_n
    assert_trips(total, [R])
    assert total % 8 != 0, "total %d takes no remainder branch of the XCD order" % total
    if rotation:
        assert S % BM == 0 and M % BM == 0, "a rotated clip of %d voxels is no whole number of %d-voxel tiles" % (S, BM)
    else:
        assert M % BM != 0, "M %d is a multiple of the tile's %d voxels" % (M, BM)
        assert S % BM != 0, "clips of %d voxels: no tile straddles two clips" % S
    return tiles_m, tiles_n, total


def gemm_sub_clips(S, tiles_n, BM, R):
    """Most whole clips a sub-launch may take so that it is at most R tiles: one trip of the loop"""
    n = (R // tiles_n) * BM // S
    assert n >= 1 and cdiv(n * S, BM) * tiles_n <= R
    return n


class GemmExpect(StreamExpect):
    """What one launch of a dense GEMM kernel must leave in its output allocation (stream_buf): StreamExpect's duties -- the
    float64 reference under `tol` relative to its abs-max, padding channels [cout, round_up(cout, 8)) exact zeros, canaries
    untouched, check_trips' bit equality with one-trip sub-launches -- with a failure placed by TILE: voxel, clip, channel,
    tile, work item, workgroup and trip of the persistent loop under a grid of R workgroups."""

    def __init__(self, want, before, ld, S, BM, BN, R, tol, guard=STREAM_GUARD):
        super().__init__(want, before, ld, S, BM, [R], tol, guard=guard)
        self.BM, self.BN, self.R = BM, BN, R
        self.tiles_n = cdiv(self.written, BN)
        self.total = cdiv(self.M, BM) * self.tiles_n

    def place(self, m, c):
        c = min(max(int(c), 0), self.tiles_n * self.BN - 1)            # a column of the row outside the launch's slice
        return gemm_place(int(m), c, self.total, self.tiles_n, self.BM, self.BN, self.R)

    def where(self, m, c=0):
        p = self.place(m, c)
        return ("voxel %d (clip %d, voxel %d of it), channel %d, tile %d (voxels from %d, channels from %d), work item %d = "
                "workgroup %d on trip %d of %d workgroups" % (m, m // self.S, m % self.S, c, p["tile"], p["m0"], p["n0"], p["item"],
                                                               p["workgroup"], p["trip"], min(self.total, self.R)))

    def tile_block(self, tile):
        """(row slice, channel slice) of a tile inside the (M, cout) reference"""
        m0, n0 = (tile // self.tiles_n) * self.BM, (tile % self.tiles_n) * self.BN
        return slice(m0, min(m0 + self.BM, self.M)), slice(n0, min(n0 + self.BN, self.C))


# ------------------------------------------------------------------ pv_mlp.hip: mlp_rows16_kernel and ln_linear_rows_kernel
# Float64 references, operands, case tables and the checker of tests/test_gpu_mlp_kernels.py.  tests/test_mlp_kernel_checks.py
# feeds the checker its own reference and defective copies of it and checks, on the CPU, every claim the tables make.
#
# An output is a (rows, ld) tensor: a launch owns channels [0, width) of the rows [r0, M) (r0 > 0: a sub-launch through offset
# pointers); the pad columns [width, ld), the rows below r0 and the MLP_EXTRA_ROWS rows behind M hold the canary.
WG_ROWS = 128                              # rows per workgroup, both kernels
MLP_WAVE_ROWS, LNL_WAVE_ROWS = 16, 32      # rows per wave: 512 threads on 16-row MFMA tiles, 256 threads on 32-row tiles
MLP_EXTRA_ROWS = 3
MLP_FORMS = {(96, 96): (3, 6), (96, 192): (3, 12), (192, 192): (6, 12), (192, 384): (6, 24), (384, 384): (12, 24)}   # (C, Cout) -> launch16<KS2, NOB16>
LNL_FORMS = {96: (6, 2), 192: (12, 2), 384: (24, 2), 768: (48, 1)}                                                    # C -> launch_ln_linear<KS, MINW>
MLP_LN_PAIRS = [p for p in MLP_FORMS if p[0] == p[1]]
BRANCH_TOL = TOL[torch.bfloat16]           # the project's bf16 bound, applied to the MLP branch alone


def row_place(m, wave_rows):
    """(workgroup, wave, row inside the wave) of row m of a launch"""
    return m // WG_ROWS, m % WG_ROWS // wave_rows, m % wave_rows


def row_layout(M, wave_rows):
    """-> (workgroups, rows held by each wave of the last workgroup)"""
    wgs = cdiv(M, WG_ROWS)
    last = M - (wgs - 1) * WG_ROWS
    return wgs, [min(max(last - w * wave_rows, 0), wave_rows) for w in range(WG_ROWS // wave_rows)]


def bf16_of(t):
    return t.to(torch.bfloat16).double()


def ref_ln64(x, gamma, beta, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def ref_mlp_rows(o, act, edit_hidden=None, **changed):
    """pv_mlp_rows in float64 on operands `o` (make_mlp_*; `changed` replaces entries): weights rounded to bf16, xn the bf16
    operand or float64 LayerNorm rounded to bf16, hidden values ref_act in float64 rounded to bf16 (edit_hidden: a defect on them).
    -> (base, branch): base = residual + b2 (LayerNorm mode: x + b2), branch = W2 . hidden."""
    o = dict(o, **changed)
    if o["ln"]:
        xn = bf16_of(ref_ln64(o["x"], o["gamma"], o["beta"], o["eps"]))
        base = o["x"].double().clone()
    else:
        xn = o["x"].to(torch.bfloat16).double()
        base = o["res"].double().clone() if o["res"] is not None else torch.zeros(xn.shape[0], o["w2"].shape[0], dtype=torch.float64)
    if o["b2"] is not None:
        base += o["b2"].double()
    pre = xn @ bf16_of(o["w1"]).t()
    if o["b1"] is not None:
        pre = pre + o["b1"].double()
    hid = bf16_of(ref_act(pre, act))
    if edit_hidden is not None:
        hid = edit_hidden(hid)
    return base, hid @ bf16_of(o["w2"]).t()


def ref_ln_linear(o, act, **changed):
    """pv_ln_linear_rows in float64: LayerNorm rounded to bf16, the Linear on bf16-rounded weights, ref_act."""
    o = dict(o, **changed)
    y = bf16_of(ref_ln64(o["x"], o["gamma"], o["beta"], o["eps"])) @ bf16_of(o["w"]).t()
    if o["b"] is not None:
        y = y + o["b"].double()
    return ref_act(y, act)


def _gelu_as_f32(x):
    """pv_gelu_fast2's operations in fp32 (Abramowitz & Stegun 7.1.25)"""
    ax = x.abs()
    t = 1.0 / ((ax * 0.70710678118654752440) * 0.47047 + 1.0)
    poly = t * (0.3480242 + t * (-0.0958798 + t * 0.7478556))
    e = torch.exp2((x * x) * -0.72134752044448170368)
    return (x + ax * (1.0 - poly * e)) * 0.5


def f32_scalar(v):
    return torch.tensor(v, dtype=torch.float32)


def replay_mlp_rows(o, act):
    """What an fp32 machine with mlp_rows16_kernel's rounding points leaves in y: LayerNorm from the mean and the centred squares,
    xn and the hidden values rounded to bf16, the A&S erf for GELU, fp32 sums on top of residual + b2 (LayerNorm mode: b2 last).
    It says how far the float64 reference itself stands from any fp32 implementation; no kernel is involved."""
    f = torch.float32
    if o["ln"]:
        x = o["x"].to(f)
        mean = x.sum(-1, keepdim=True) * f32_scalar(1.0 / x.shape[1])
        var = ((x - mean) ** 2).sum(-1, keepdim=True) * f32_scalar(1.0 / x.shape[1])
        xn = ((x - mean) * torch.rsqrt(var + f32_scalar(o["eps"])) * o["gamma"].to(f) + o["beta"].to(f)).to(torch.bfloat16).to(f)
        y = x.clone()
    else:
        xn = o["x"].to(torch.bfloat16).to(f)
        y = o["res"].to(f).clone() if o["res"] is not None else torch.zeros(xn.shape[0], o["w2"].shape[0], dtype=f)
        if o["b2"] is not None:
            y += o["b2"].to(f)
    pre = xn @ o["w1"].to(torch.bfloat16).to(f).t()
    if o["b1"] is not None:
        pre = pre + o["b1"].to(f)
    if act == L.ACT_GELU:
        hid = _gelu_as_f32(pre)
    elif act == L.ACT_RELU:
        hid = pre.clamp_min(0)
    elif act == L.ACT_SWISH:
        hid = pre * torch.sigmoid(pre)
    elif act == L.ACT_SIGMOID:
        hid = torch.sigmoid(pre)
    else:
        hid = pre
    y = y + hid.to(torch.bfloat16).to(f) @ o["w2"].to(torch.bfloat16).to(f).t()
    if o["ln"]:
        y = y + o["b2"].to(f)
    return y


def _mlp_float_operands(C, H, Cout, M, seed):
    g = torch.Generator().manual_seed(seed)
    o = dict(C=C, H=H, Cout=Cout, M=M, eps=1e-6)
    o["w1"] = (torch.randn(H, C, generator=g) * C ** -0.5).bfloat16().float()
    o["w2"] = (torch.randn(Cout, H, generator=g) * H ** -0.5).bfloat16().float()
    o["b1"], o["b2"] = torch.randn(H, generator=g) * 0.3, torch.randn(Cout, generator=g) * 0.3
    o["gamma"], o["beta"] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    o["x32"] = torch.randn(M, C, generator=g) * 2.0 + 3.0 * torch.randn(M, 1, generator=g)      # rows with a large mean
    o["r32"] = torch.randn(M, Cout, generator=g)
    o["nn_gamma"], o["nn_beta"] = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    return o


def make_mlp_float(C, H, Cout, ln, res, M, seed=77):
    """Seeded normal operands, drawn as tests/test_gpu_kernels.py::test_fused_mlp_rows draws them."""
    o = _mlp_float_operands(C, H, Cout, M, seed)
    x32, r32 = o.pop("x32"), o.pop("r32")
    o.update(ln=ln, x=x32 if ln else x32.bfloat16(), res=r32 if (res and not ln) else None)
    return o


def make_mlp_int(C, H, Cout, ln, M, seed=1301):
    """Operands under which every value of the launch is an integer that its format holds exactly (mlp_int_conditions): the
    output equals the float64 reference bit for bit in any summation order."""
    g = torch.Generator().manual_seed(seed + C + 7 * H + 13 * Cout)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    o = dict(C=C, H=H, Cout=Cout, M=M, ln=ln, eps=1e-6)
    p0 = ri(0, C - 1, (H,))
    p1 = (p0 + ri(1, C - 1, (H,))) % C                                   # a second, different channel
    w1 = torch.zeros(H, C)
    w1[torch.arange(H), p0] = (2 * ri(0, 1, (H,)) - 1).float()
    w1[torch.arange(H), p1] = (2 * ri(0, 1, (H,)) - 1).float()
    o["w1"], o["w2"] = w1, ri(-2, 2, (Cout, H)).float()
    o["b1"], o["b2"] = 16.0 * ri(-3, 3, (H,)), 16.0 * ri(-3, 3, (Cout,))
    if ln:
        # gamma = 0: xn is beta for every row, whatever the statistics; 193 is prime, so channels 8, 16 or 32 apart differ
        o["gamma"], o["beta"] = torch.zeros(C), 16.0 * ((torch.arange(C) * 37 + seed) % 193 - 96)
        o["x"], o["res"] = ri(-64, 64, (M, C)).float(), None             # the residual: another integer row per token
    else:
        o["gamma"] = o["beta"] = None
        o["x"], o["res"] = (16.0 * ri(-8, 8, (M, C))).bfloat16(), 16.0 * ri(-8, 8, (M, Cout))
    o["nn_gamma"], o["nn_beta"] = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    return o


def mlp_int_conditions(o, acts):
    """The conditions under which an integer case is exact, asserted on its operands: xn exact in bf16; every pre-activation a
    multiple of 16 (pv_gelu_fast2 is exact at 0 and from |x| = 16 on: exp2f(-0.7213 * 256) is 0, what is left is (x + |x|) / 2);
    hidden values at most 256 * 16, exact in bf16; every partial sum below 2^24 in magnitude, exact in fp32."""
    xn = (o["beta"].expand(o["M"], -1) if o["ln"] else o["x"]).double()
    assert o["ln"] is False or not o["gamma"].any()
    assert torch.equal(bf16_of(xn), xn) and torch.equal(bf16_of(o["w1"]), o["w1"].double()) and torch.equal(bf16_of(o["w2"]), o["w2"].double())
    assert ((o["w1"] != 0).sum(1) == 2).all() and (o["w1"].abs() <= 1).all() and (o["w2"].abs() <= 2).all()
    pre = xn @ o["w1"].double().t() + o["b1"].double()
    assert (pre % 16 == 0).all() and (xn.abs() @ o["w1"].abs().double().t() + o["b1"].abs().double()).max() < 2 ** 24
    worst = 0.0
    for act in acts:
        assert act in (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU)
        hid = ref_act(pre, act)
        assert torch.equal(hid, pre if act == L.ACT_NONE else pre.clamp_min(0)), "the float64 activation is not exact here"
        assert hid.abs().max() <= 256 * 16 and torch.equal(bf16_of(hid), hid)
        base, _ = ref_mlp_rows(o, act)
        total = (hid.abs() @ o["w2"].abs().double().t() + (o["x"].abs().double() if o["ln"] else o["res"].abs().double())
                 + o["b2"].abs().double()).max().item()
        assert total < 2 ** 24 and (base % 1 == 0).all()
        worst = max(worst, total)
    return worst


# A2: name -> (C, H, Cout, LayerNorm mode, residual, activation, M).  All five (C, Cout) pairs in operand mode and the three
# C == Cout pairs in LayerNorm mode with GELU (the instantiations MViT launches), SWISH and SIGMOID through the runtime-activation
# instantiation; H = 32, 96, 160 (1, 3, 5 hidden blocks) and M = 1, 15, 17, 127, 128, 129, 273 spread over them.
MLP_A2 = {
    "op_96_96": (96, 32, 96, False, True, L.ACT_GELU, 1),
    "op_96_192": (96, 96, 192, False, True, L.ACT_GELU, 273),
    "op_192_192": (192, 160, 192, False, False, L.ACT_GELU, 17),
    "op_192_384": (192, 32, 384, False, True, L.ACT_GELU, 127),
    "op_384_384": (384, 96, 384, False, False, L.ACT_GELU, 128),
    "ln_96": (96, 160, 96, True, False, L.ACT_GELU, 129),
    "ln_192": (192, 32, 192, True, False, L.ACT_GELU, 273),
    "ln_384": (384, 96, 384, True, False, L.ACT_GELU, 273),
    "op_192_384_swish": (192, 160, 384, False, True, L.ACT_SWISH, 15),
    "ln_384_sigmoid": (384, 160, 384, True, False, L.ACT_SIGMOID, 129),
}
MLP_A1_H = (32, 64, 96, 160, 224)          # 1, 2, 3, 5, 7 hidden blocks: the ring wraps at 3; at 7 every buffer has been reused twice
MLP_A1_M = 273                             # two full workgroups, then wave 0 full, wave 1 with one row, waves 2-7 empty
MLP_A1_ACTS = (L.ACT_GELU, L.ACT_NONE, L.ACT_RELU)
MLP_A3_ROWS = {0: "constant", 5: "variance_eps", 16: "outlier_first", 20: "outlier_last"}   # row of the launch -> edge; M = 21
MLP_A3_M = 21
MLP_RANGES = (1, 129, 256 + 16)            # A6: the launches of rows [r0, M)
LNL_RANGES = (1, 129)
LNL_B1_N = (32, 64, 96, 160)               # 1, 2, 3, 5 output blocks
LNL_B4_M = (1, 31, 33, 97, 128, 129, 161, 193)
LNL_ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH, L.ACT_GELU, L.ACT_SIGMOID)


def ln_edge_row(kind, C, seed=5):
    """The LayerNorm edge rows: a constant row (variance 0); a row of +-1e-3 (variance 1e-6, the size of ln_eps); a normal row
    with one outlier of 1e3 in channel 0 (ln_linear_rows_kernel's shift) or in the last channel."""
    g = torch.Generator().manual_seed(seed + C)
    if kind == "constant":
        return torch.full((C,), 3.5)
    if kind == "variance_eps":
        sign = torch.ones(C)
        sign[torch.randperm(C, generator=g)[:C // 2]] = -1.0
        return 1e-3 * sign
    row = torch.randn(C, generator=g)
    row[0 if kind == "outlier_first" else C - 1] = 1e3
    return row


def make_mlp_edges(C, H, eps, seed=79):
    """A3: LayerNorm mode, C = Cout, normal rows with the edge rows of MLP_A3_ROWS among them."""
    o = make_mlp_float(C, H, C, True, False, MLP_A3_M, seed)
    for m, kind in MLP_A3_ROWS.items():
        o["x"][m] = ln_edge_row(kind, C)
    o["eps"] = eps
    return o


def make_lnl_float(C, N, M, seed=78):
    """Seeded normal operands, drawn as test_layernorm_fused_into_the_qkv_linear draws them."""
    g = torch.Generator().manual_seed(seed)
    o = dict(C=C, N=N, M=M, eps=1e-6)
    o["w"] = (torch.randn(N, C, generator=g) * C ** -0.5).bfloat16().float()
    o["b"] = torch.randn(N, generator=g) * 0.3
    o["gamma"], o["beta"] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    o["x"] = torch.randn(M, C, generator=g) * 2.0 + 5.0 * torch.randn(M, 1, generator=g)
    return o


def make_lnl_int(C, N, M, seed=1401):
    """B1: gamma = 0 and an integer beta (period 97, a prime: channels 8, 16 or 32 apart differ), W in {-1, 0, 1} with at most four
    non-zeros per row, an integer bias: every output is an integer of magnitude <= 4 * 48 + 60 <= 256, exact in bf16."""
    o = make_lnl_float(C, N, M, seed)
    g = torch.Generator().manual_seed(seed + C + 3 * N)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    o["gamma"], o["beta"] = torch.zeros(C), ((torch.arange(C) * 37 + seed) % 97 - 48).float()
    w = torch.zeros(N, C)
    for _ in range(4):
        w[torch.arange(N), ri(0, C - 1, (N,))] = (2 * ri(0, 1, (N,)) - 1).float()
    o["w"], o["b"] = w, ri(-60, 60, (N,)).float()
    return o


def lnl_int_conditions(o):
    assert not o["gamma"].any() and torch.equal(bf16_of(o["beta"]), o["beta"].double())
    nz = (o["w"] != 0).sum(1)
    assert (nz >= 1).all() and (nz <= 4).all() and (o["w"].abs() <= 1).all() and (o["b"] % 1 == 0).all()
    want = ref_ln_linear(o, L.ACT_NONE)
    assert (want % 1 == 0).all() and want.abs().max() <= 256 and torch.equal(bf16_of(want), want)
    assert (o["beta"].abs().double() @ o["w"].abs().double().t() + o["b"].abs().double()).max() <= 256
    return want.abs().max().item()


def make_lnl_select(C, M, seed=1501):
    """B2: W one-hot under a seeded permutation sigma (N = C), no bias, gamma = 1, beta = 0: y[m][n] is the normalised channel
    sigma(n) of row m.  The rows are normal rows with a large mean and the LayerNorm edge rows at 0, 33 (wave 1), M - 2, M - 1."""
    o = make_lnl_float(C, C, M, seed)
    g = torch.Generator().manual_seed(seed + C)
    o["sigma"] = torch.randperm(C, generator=g)
    w = torch.zeros(C, C)
    w[torch.arange(C), o["sigma"]] = 1.0
    o["w"], o["b"], o["gamma"], o["beta"] = w, None, torch.ones(C), torch.zeros(C)
    o["edges"] = {0: "outlier_first", 33: "constant", M - 2: "variance_eps", M - 1: "outlier_last"}
    for m, kind in o["edges"].items():
        o["x"][m] = ln_edge_row(kind, C)
    return o


def _explain_by_hidden(d, w2):
    """Integer cases: the error row d (Cout,) of one token is W2 times the error of its hidden values.  Name the hidden unit, or
    the hidden block, whose columns of W2 span it."""
    w2, d = w2.double(), d.double()
    alpha = (d @ w2) / (w2 * w2).sum(0).clamp_min(1.0)
    resid = (d[:, None] - w2 * alpha[None, :]).abs().max(0).values
    u = int(resid.argmin())
    if resid[u] < 1e-6 and alpha[u] != 0:
        return "explained by hidden unit %d alone (hidden block %d, unit %d of it) being off by %g" % (u, u // 32, u % 32, alpha[u])
    for hb in range(w2.shape[1] // 32):
        a = w2[:, 32 * hb:32 * hb + 32]
        sol = torch.linalg.lstsq(a, d[:, None]).solution
        if (a @ sol - d[:, None]).abs().max() < 1e-6 * max(1.0, d.abs().max().item()):
            return "explained by the units of hidden block %d alone" % hb
    return "not explained by the units of any single hidden block"


class MlpExpect:
    """What one launch of mlp_rows16_kernel (wave_rows 16) or ln_linear_rows_kernel (wave_rows 32, base None) must leave in its
    output, on the Expect pattern: a buffer with canaries, the owned rows [r0, M), the written width.

    base, branch  (M, width) float64: the launch must leave base + branch, and the error is measured on got - base against the
                  branch ALONE, relative to the branch's abs-max (a residual stream many times the branch hides it otherwise)
    before        the (rows, ld) buffer as it was handed to the launch
    tol           bound on max|got - base - branch| / max|branch|; None (and no per_elem): bit-equal to base + branch in the
                  buffer's dtype
    per_elem      (rel, floor) instead: |got - base - branch| <= rel * |branch| + floor * max|branch| for every element
    w2            integer cases: the failure also names the hidden unit or block that explains the worst row's error
    """

    def __init__(self, base, branch, before, ld, M, r0=0, wave_rows=MLP_WAVE_ROWS, tol=None, per_elem=None, w2=None):
        self.branch = branch.cpu().double()
        self.base = torch.zeros_like(self.branch) if base is None else base.cpu().double()
        self.before, self.ld, self.M, self.r0, self.wave_rows = before.cpu().clone(), ld, M, r0, wave_rows
        self.tol, self.per_elem, self.w2 = tol, per_elem, w2
        self.width = self.branch.shape[1]
        assert self.branch.shape == self.base.shape == (M, self.width) and 0 <= r0 < M
        assert self.before.dim() == 2 and self.before.shape[0] >= M and self.before.shape[1] == ld >= self.width

    def where(self, m, c):
        wg, wave, row = row_place(m - self.r0, self.wave_rows)
        return "row %d (workgroup %d, wave %d, lane row %d of the launch from row %d), channel %d" % (m, wg, wave, row, self.r0, c)

    def ideal(self, base=None, branch=None):
        """The buffer a kernel that computes the reference exactly leaves (or `base` + `branch` in its place)."""
        buf = self.before.clone()
        want = (self.base if base is None else base) + (self.branch if branch is None else branch)
        buf[self.r0:self.M, :self.width] = want[self.r0:].to(buf.dtype)
        return buf

    def check(self, got, what=""):
        """-> the error of the branch relative to its abs-max"""
        got = got.detach().cpu()
        assert got.shape == self.before.shape and got.dtype == self.before.dtype, what
        rows = slice(self.r0, self.M)
        data, base, branch = got[rows, :self.width], self.base[rows], self.branch[rows]
        diff = (data.double() - base - branch).abs()
        diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
        scale = max(branch.abs().max().item(), 1e-6)
        err = diff.max().item() / scale
        if self.per_elem is not None:
            over = diff - (self.per_elem[0] * branch.abs() + self.per_elem[1] * scale)
            bad, reason = over > 0, "beyond %g |want| + %g max|want|" % self.per_elem
            diff = over
        elif self.tol is not None:
            bad, reason = diff > self.tol * scale, "error %.3e of the branch abs-max > %.1e" % (err, self.tol)
        else:
            bad, reason = data != (base + branch).to(got.dtype), "must be bit-equal to the reference"
        if bad.any():
            flat = int(torch.where(bad, diff, torch.full_like(diff, -1.0)).argmax())
            m, c = self.r0 + flat // self.width, flat % self.width
            msg = "%s: %d elements of %d rows %s; worst at %s: %r against %r" % (
                what, bad.sum().item(), bad.any(1).sum().item(), reason, self.where(m, c), got[m, c].item(),
                (self.base[m, c] + self.branch[m, c]).item())
            if self.w2 is not None:
                msg += "; the row's error is " + _explain_by_hidden(got[m, :self.width].double() - self.base[m] - self.branch[m], self.w2)
            raise AssertionError(msg)
        rest_got, rest_before = got.clone(), self.before.clone()
        rest_got[rows, :self.width] = 0
        rest_before[rows, :self.width] = 0
        ne = rest_got != rest_before
        if ne.any():
            m, c = (int(v) for v in ne.nonzero()[0])
            kind = "a pad column" if c >= self.width else ("a row at or behind M = %d" % self.M if m >= self.M else "a row below the launch's first")
            raise AssertionError("%s: %d elements the launch does not own changed, first at row %d, column %d (%s)" % (
                what, ne.sum().item(), m, c, kind))
        return err

    def same_bits(self, a, b, what="", r0_b=None):
        """The owned part of two outputs of the same rows, bit for bit (b a launch from row r0_b: its rows sit in other lanes,
        waves and workgroups).  A row's value comes from the same instructions in the same order wherever it sits."""
        a, b = a.detach().cpu(), b.detach().cpu()
        r0_b = self.r0 if r0_b is None else r0_b
        lo = max(self.r0, r0_b)
        ne = a[lo:self.M, :self.width] != b[lo:self.M, :self.width]
        if ne.any():
            m = lo + int(ne.any(1).nonzero()[0])
            c = int(ne[m - lo].nonzero()[0])
            pa, pb = row_place(m - self.r0, self.wave_rows), row_place(m - r0_b, self.wave_rows)
            raise AssertionError("%s: %d elements of %d rows differ; first at row %d, channel %d: %r as (workgroup, wave, lane row) "
                                 "%r against %r as %r" % (what, ne.sum().item(), ne.any(1).sum().item(), m, c, a[m, c].item(), pa,
                                                          b[m, c].item(), pb))


# ------------------------------------------------------------------ csrc/pv_attn.hip, pv_attn64.hip (pv_attention)
# Float64 references, operand families, the mirror of the deferred-rescale rule, an fp32 replay of the kernels' arithmetic and
# the checker of tests/test_gpu_attention_kernels.py.  tests/test_attention_kernel_checks.py feeds the checker its own reference
# and defective replays and checks, on the CPU, every claim the families make.
#
# Operands are (B, N, heads, D) tensors of values the storage type holds exactly.  AttnLayout says where they lie: every
# operand is a flat buffer, item b of operand x starts at off[x] + b * bs[x], row n of it at + n * ld[x], head h at + h * D.
ATTN_WG_ROWS, ATTN_WAVE_ROWS = 128, 32     # kQB / kRowsWG; one 32-row block per wave
ATTN_DEFER = 8.0                           # kDefer
ATTN_LOG2E_F32 = 1.44269504088896340736    # the literal the kernels multiply d.scale by (as fp32)
ATTN_INT_SCALE = 0.08664339780807495       # families A and B: fp32(scale) * fp32(log2 e) == 0.125 exactly
ATTN_GUARD_TILES = 6                       # NaN rows behind the last item of Q, K and V, in key tiles
ATTN_ROUTES = {                            # (dtype, head_dim) -> (routed symbol, instantiation)
    (torch.bfloat16, 96): ("attn_w64_kernel", "attn_w64_kernel"),
    (torch.bfloat16, 64): ("attn_pipe_kernel", "attn_pipe_kernel<64>"),
    (torch.bfloat16, 32): ("attn_pipe_kernel", "attn_pipe_kernel<32>"),
    (torch.bfloat16, 128): ("attn_kernel", "attn_kernel<bf16_t, 128>"),
    (torch.float32, 32): ("attn_kernel", "attn_kernel<float, 32>"),
    (torch.float32, 64): ("attn_kernel", "attn_kernel<float, 64>"),
    (torch.float32, 96): ("attn_kernel", "attn_kernel<float, 96>"),
    (torch.float32, 128): ("attn_kernel", "attn_kernel<float, 128>"),
}
ATTN_NOT_LAUNCHED = ("attn_kernel<bf16_t, 32>", "attn_kernel<bf16_t, 64>", "attn_kernel<bf16_t, 96>")   # K / V beyond 2 GiB only
# 1, 1, 1, 1, 2, 2, 3, 4, 7, 8 (ragged), 8 tiles: both tail forms of the loop unrolled by two, two trips of it, every
# (t & 1, t % 3) pair in a `more` step (t = 0 .. 6)
ATTN_NK = {64: (1, 3, 37, 64, 65, 128, 192, 256, 448, 485, 512), 32: (1, 3, 19, 32, 33, 64, 96, 128, 224, 243, 256)}
ATTN_TILES = (1, 1, 1, 1, 2, 2, 3, 4, 7, 8, 8)


def attn_kt(dtype):
    return 64 if dtype == torch.bfloat16 else 32


def attn_step_form(t, Nk, KT):
    """The form of the tile step that consumes key tile t (pv_attn64.hip / attn_pipe_kernel; attn_kernel has one loop body, for
    which the same words name the tile's place in it)."""
    nt = cdiv(Nk, KT)
    if t + 1 < nt:
        form = "`more` step, parity %d, V slot %d" % (t & 1, t % 3)
    else:
        form = "ragged last step" if Nk % KT else "last step"
    return form + (", scores from the prologue" if t == 0 else "")


def attn_log2_scale(scale):
    """The factor of the exp2 domain as the kernels form it: fp32(scale) * fp32(log2 e), one fp32 rounding."""
    f = torch.tensor(scale, dtype=torch.float32) * torch.tensor(ATTN_LOG2E_F32, dtype=torch.float32)
    return float(f)


def ref_attention(q, k, v, log2_scale, residual_q):
    """float64 softmax attention in the exp2 domain: weights 2^(log2_scale * q.k).  -> ((B, Nq, H, D) output, (B, H, Nq) index of
    each row's dominant key)"""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * log2_scale
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    o = torch.einsum("bhqk,bkhd->bqhd", p / p.sum(-1, keepdim=True), v)
    return (o + q if residual_q else o), s.argmax(-1)


def _attn_pad_rows(x, w64):
    """Rows of one (batch, head) filled up to whole waves the way the kernels fill their idle lanes: attn_w64_kernel repeats row
    Nq - 1, the others hold zeros."""
    n = x.shape[0]
    pad = cdiv(n, ATTN_WAVE_ROWS) * ATTN_WAVE_ROWS - n
    if not pad:
        return x
    fill = x[-1:].expand(pad, -1) if w64 else torch.zeros(pad, x.shape[1], dtype=x.dtype)
    return torch.cat([x, fill])


def attn_mirror(args, KT, w64):
    """The deferred-rescale rule alone, on the (Nq, Nk) exponent arguments of one (batch, head): per wave of 32 rows, m_run from
    a full first tile for attn_w64_kernel and from -1e30 otherwise, advanced where __any(mx > m_run + kDefer).  Coverage only --
    no expected value comes from here.  -> list of events dict(wave, t, rescaled, rise (per lane, above the held maximum; None
    before the first finite maximum), stale (largest argument above the maximum held AFTER the decision))"""
    Nq, Nk = args.shape
    a = _attn_pad_rows(args.double(), w64)
    nt, ev = cdiv(Nk, KT), []
    for w in range(a.shape[0] // ATTN_WAVE_ROWS):
        rows = a[w * ATTN_WAVE_ROWS:(w + 1) * ATTN_WAVE_ROWS]
        m = torch.full((ATTN_WAVE_ROWS,), -1e30, dtype=torch.float64)
        if w64 and KT <= Nk:
            m = rows[:, :KT].max(1).values
        for t in range(nt):
            mx = rows[:, t * KT:min((t + 1) * KT, Nk)].max(1).values
            started = bool((m > -1e29).all())
            rise = mx - m
            trip = bool((mx > m + ATTN_DEFER).any())
            if trip:
                m = torch.maximum(m, mx)
            ev.append(dict(wave=w, t=t, rescaled=trip, rise=rise if started else None, stale=float((mx - m).max())))
    return ev


def attn_mirror_coverage(events, Nk, KT):
    """What a list of mirror events contains, as a set of names (the list family B must cover per route)."""
    nt, got = cdiv(Nk, KT), set()
    for e in events:
        if e["rise"] is None:
            continue
        top = float(e["rise"].max())
        if not e["rescaled"] and top == ATTN_DEFER:
            got.add("no rescale at a rise of exactly 8")
        if e["rescaled"] and top == ATTN_DEFER + 1:
            got.add("rescale at a rise of 9")
        if e["stale"] == ATTN_DEFER:
            got.add("stale P of 2^8")
        if e["rescaled"]:
            over = e["rise"] > ATTN_DEFER
            if over.sum() == 1 and ((e["rise"] > 0) & ~over).sum() >= 8:
                got.add("one-lane rescale")
            if top <= 12:     # a moderate alpha, 2^-1 .. 2^-12 on the lane that rose most
                got.add(("rescale in a " + attn_step_form(e["t"], Nk, KT)).split(", V slot")[0].split(", scores")[0])
    return got


ATTN_B_COVER = {"no rescale at a rise of exactly 8", "rescale at a rise of 9", "stale P of 2^8", "one-lane rescale",
                "rescale in a `more` step, parity 0", "rescale in a `more` step, parity 1", "rescale in a last step",
                "rescale in a ragged last step"}
ATTN_DEFECTS = ("swap_v", "stale_v", "alpha_l", "pair_l", "mask_short", "mask_long", "halves", "head")


def replay_attention(q, k, v, log2_scale, residual_q, dtype, w64, defect=None):
    """fp32 replay of the kernels' arithmetic: KT-key tiles, online softmax in the exp2 domain with the deferred rescale decided
    per 32-row wave, P rounded to bf16 for the PV product (bf16 routes), l from the unrounded p, one rounding at the end.
    defect: one of ATTN_DEFECTS --
      swap_v      keys 5 and 6 of every 16-key slot read each other's V row
      stale_v     from tile 3 on a tile's V comes from three tiles earlier (a V ring slot not rewritten)
      alpha_l     alpha not applied to l in any rescale after a row's first
      pair_l      the first pair of p of every tile missing from l
      mask_short  key Nk - 1 masked too;  mask_long  key Nk (a zero row, score 0) not masked
      halves      the two lane halves (keys with bit 2 clear / set) each keep their own running maximum
      head        head h reads K and V of head h + 1 (the last one of head 0)
    -> (B, Nq, H, D) in `dtype`"""
    f32 = torch.float32
    bf16 = dtype == torch.bfloat16
    KT = attn_kt(dtype)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    nt = cdiv(Nk, KT)
    sc = torch.tensor(log2_scale, dtype=f32)
    out = torch.empty(B, Nq, H, D, dtype=dtype)
    half_of_key = ((torch.arange(KT) >> 2) & 1).bool()            # crow(r, hi): the keys of lane half 1 have bit 2 set
    half_of_chan = ((torch.arange(D) >> 2) & 1).bool()            # d0 = db * 32 + 8 g + 4 hi
    for b in range(B):
        for h in range(H):
            hk = (h + 1) % H if defect == "head" else h
            qq = _attn_pad_rows(q[b, :, h].to(f32), w64)
            R = qq.shape[0]
            kk = torch.zeros(nt * KT, D, dtype=f32)
            vv = torch.zeros(nt * KT, D, dtype=f32)
            kk[:Nk], vv[:Nk] = k[b, :, hk].to(f32), v[b, :, hk].to(f32)
            valid = torch.arange(nt * KT) < (Nk - 1 if defect == "mask_short" else Nk + 1 if defect == "mask_long" else Nk)
            nh = 2 if defect == "halves" else 1
            m = torch.full((R, nh), -1e30, dtype=f32)
            if w64 and KT <= Nk:
                s0 = (qq @ kk[:KT].T) * sc
                m = torch.stack([s0[:, ~half_of_key].max(1).values, s0[:, half_of_key].max(1).values], 1) if nh == 2 \
                    else s0.max(1, keepdim=True).values
            l = torch.zeros(R, nh, dtype=f32)
            o = torch.zeros(R, D, dtype=f32)
            first = torch.ones(R, dtype=torch.bool)
            for t in range(nt):
                ks = slice(t * KT, (t + 1) * KT)
                s = qq @ kk[ks].T
                s = torch.where(valid[ks][None, :], s, torch.full_like(s, -1e30))
                if nh == 2:
                    mx = torch.stack([s[:, ~half_of_key].max(1).values, s[:, half_of_key].max(1).values], 1) * sc
                else:
                    mx = s.max(1, keepdim=True).values * sc
                trip = (mx > m + ATTN_DEFER).any(1).view(-1, ATTN_WAVE_ROWS).any(1).repeat_interleave(ATTN_WAVE_ROWS)
                m_new = torch.where(trip[:, None], torch.maximum(m, mx), m)
                alpha = torch.exp2(m - m_new)
                m = m_new
                l = l * (torch.where(first[:, None], alpha, torch.ones_like(alpha)) if defect == "alpha_l" else alpha)
                first = first & ~trip
                o = o * (torch.where(half_of_chan[None, :], alpha[:, 1:2], alpha[:, 0:1]) if nh == 2 else alpha)
                mk = torch.where(half_of_key[None, :], m[:, 1:2], m[:, 0:1]) if nh == 2 else m
                p = torch.exp2(s * sc - mk)
                pl = p.clone()
                if defect == "pair_l":
                    pl[:, :2] = 0
                if nh == 2:
                    l = l + torch.stack([pl[:, ~half_of_key].sum(1), pl[:, half_of_key].sum(1)], 1)
                else:
                    l = l + pl.sum(1, keepdim=True)
                vt = vv[slice((t - 3) * KT, (t - 2) * KT) if defect == "stale_v" and t >= 3 else ks]
                if defect == "swap_v":
                    idx = torch.arange(KT)
                    idx[5::16], idx[6::16] = torch.arange(6, KT, 16), torch.arange(5, KT, 16)
                    vt = vt[idx]
                o = o + (p.to(torch.bfloat16).to(f32) if bf16 else p) @ vt
            res = o * (1.0 / l.sum(1, keepdim=True))
            if residual_q:
                res = res + qq
            out[b, :, h] = res[:Nq].to(dtype)
    return out


class AttnLayout:
    """Where the operands of one pv_attention case lie.
      packed  ld = heads * D, items back to back, one buffer per operand
      wide    ldq, ldk, ldv, ldo all different and wider than heads * D, three spare rows and a different odd gap behind every item
      fused   q, k and v are channel slices of ONE buffer of rows 3 * heads * D + 8 wide; o as in `wide`
    Every element of Q, K and V that is not an operand value is NaN: the channels past the width, the rows between items and
    ATTN_GUARD_TILES key tiles of rows behind the last item.  Every element of O is the canary."""

    def __init__(self, kind, B, H, D, Nq, Nk, dtype):
        self.kind, self.B, self.H, self.D, self.Nq, self.Nk, self.dtype = kind, B, H, D, Nq, Nk, dtype
        W, guard = H * D, ATTN_GUARD_TILES * attn_kt(dtype)
        n = dict(q=Nq, k=Nk, v=Nk, o=Nq)
        self.off = dict(q=0, k=0, v=0, o=0)
        if kind == "packed":
            self.ld = dict.fromkeys("qkvo", W)
            self.bs = {x: n[x] * W for x in "qkvo"}
        else:
            self.ld = dict(q=W + 8, k=W + 16, v=W + 24, o=W + 32)
            self.bs = {x: (n[x] + 3) * self.ld[x] + 8 * (i + 1) for i, x in enumerate("qkvo")}
            if kind == "fused":
                ld = 3 * W + 8
                self.ld.update(q=ld, k=ld, v=ld)
                self.bs.update(dict.fromkeys("qkv", (max(Nq, Nk) + 3) * ld + 8))
                self.off.update(k=W, v=2 * W)
        rows = {x: (max(Nq, Nk) if kind == "fused" and x != "o" else n[x]) + (3 if x == "o" else guard) for x in "qkvo"}
        self.size = {x: (B - 1) * self.bs[x] + rows[x] * self.ld[x] for x in "qkvo"}

    def view(self, buf, x, b=None, h=None, rows=None):
        """the (items, rows, heads, D) elements of operand x inside its flat buffer (a strided view)"""
        b, h = b or (0, self.B), h or (0, self.H)
        rows = rows or (0, self.Nq if x in "qo" else self.Nk)
        off = self.off[x] + b[0] * self.bs[x] + rows[0] * self.ld[x] + h[0] * self.D
        return buf.as_strided((b[1] - b[0], rows[1] - rows[0], h[1] - h[0], self.D), (self.bs[x], self.ld[x], self.D, 1), off)

    def inputs(self, q, k, v):
        """-> {"q", "k", "v"}: flat NaN-filled buffers holding the operands (one shared buffer when fused)"""
        nan = float("nan")
        if self.kind == "fused":
            one = torch.full((self.size["q"],), nan, dtype=self.dtype)
            bufs = dict(q=one, k=one, v=one)
        else:
            bufs = {x: torch.full((self.size[x],), nan, dtype=self.dtype) for x in "qkv"}
        for x, t in (("q", q), ("k", k), ("v", v)):
            assert (t.to(self.dtype).double() == t.double()).all(), "operand %s is not exact in %s" % (x, self.dtype)
            self.view(bufs[x], x).copy_(t.to(self.dtype))
        return bufs

    def output(self):
        return torch.full((self.size["o"],), CANARY, dtype=self.dtype)


class AttnExpect:
    """What one launch of pv_attention must leave in its output buffer.

    want    (B, Nq, H, D) float64 reference;  dom  (B, H, Nq) the dominant key of every row (ref_attention gives both)
    lay     the AttnLayout;  route  the routed symbol
    mode    "bits": bit-equal to want in the buffer's dtype;  "elem": |got - want| <= bound |want| per element;
            "row": max|got - want| over a query row / max|want| over that row <= bound
    b, h, rows  the sub-range the launch owns (default everything): every other element of O keeps the canary
    A failure names batch item, head, query row, workgroup, wave and lane, channel and channel block, and the key tile and step
    form the row's dominant key lies in."""

    def __init__(self, want, dom, lay, route, mode, bound=None, b=None, h=None, rows=None):
        self.want, self.dom, self.lay, self.route, self.mode, self.bound = want.double(), dom, lay, route, mode, bound
        self.b, self.h, self.rows = b or (0, lay.B), h or (0, lay.H), rows or (0, lay.Nq)
        assert mode in ("bits", "elem", "row") and (bound is None) == (mode == "bits")
        assert self.want.shape == (lay.B, lay.Nq, lay.H, lay.D) and self.rows[0] % ATTN_WG_ROWS == 0

    def _own(self, t):
        return t[self.b[0]:self.b[1], self.rows[0]:self.rows[1], self.h[0]:self.h[1]]

    def where(self, b, m, h, c):
        lay, KT = self.lay, attn_kt(self.lay.dtype)
        r = m - self.rows[0]
        j = int(self.dom[b, h, m])
        nqb = cdiv(self.rows[1] - self.rows[0], ATTN_WG_ROWS)
        item = ((b - self.b[0]) * (self.h[1] - self.h[0]) + h - self.h[0]) * nqb + r // ATTN_WG_ROWS
        hi = (c >> 2) & 1
        return ("batch item %d, head %d, query row %d (work item %d of the launch, query block %d, wave %d, lane %d), channel %d "
                "(channel block %d, lane half %d); %s, Nk = %d: the row's dominant key %d is in key tile %d (16-key slot %d, "
                "lane half %d), consumed by the %s" % (
                    b, h, m, item, r // ATTN_WG_ROWS, r % ATTN_WG_ROWS // ATTN_WAVE_ROWS, r % ATTN_WAVE_ROWS + 32 * hi, c,
                    c // 32, hi, self.route, lay.Nk, j, j // KT, j % KT // 16, (j >> 2) & 1, attn_step_form(j // KT, lay.Nk, KT)))

    def ideal(self, values=None):
        """The buffer a kernel that computes the reference (or `values`, (B, Nq, H, D)) exactly leaves."""
        buf = self.lay.output()
        self.lay.view(buf, "o", self.b, self.h, self.rows).copy_(self._own(self.want if values is None else values).to(buf.dtype))
        return buf

    def values(self, buf):
        return self.lay.view(buf.detach().cpu(), "o", self.b, self.h, self.rows).clone()

    def check(self, got, what=""):
        """-> the worst error in the mode's own metric (0 for "bits")"""
        got = got.detach().cpu()
        assert got.shape == (self.lay.size["o"],) and got.dtype == self.lay.dtype, what
        data, want = self.values(got), self._own(self.want)
        diff = (data.double() - want).abs()
        diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
        if self.mode == "bits":
            over, reason = (data != want.to(got.dtype)).double(), "must be bit-equal to the reference"
            err = 0.0
        elif self.mode == "elem":
            rel = diff / want.abs().clamp_min(1e-300)
            over, err = diff - self.bound * want.abs(), rel.max().item()
            reason = "beyond %.3e |want| (worst %.3e)" % (self.bound, err)
        else:
            rel = diff.max(-1, keepdim=True).values / want.abs().max(-1, keepdim=True).values.clamp_min(1e-30)
            over, err = (rel - self.bound).expand_as(diff) * (diff == diff.max(-1, keepdim=True).values), rel.max().item()
            reason = "are the worst of a query row beyond %.1e of the row's own abs-max (worst row %.3e)" % (self.bound, err)
        bad = over > 0
        if bad.any():
            flat = int(torch.where(bad, over, torch.full_like(over, -1.0)).argmax())
            nb, nr, nh, D = data.shape
            b, m, h, c = flat // (nr * nh * D), flat // (nh * D) % nr, flat // D % nh, flat % D
            raise AssertionError("%s: %d elements of %d rows %s; worst at %s: %r against %r" % (
                what, bad.sum().item(), bad.any(-1).sum().item(), reason,
                self.where(b + self.b[0], m + self.rows[0], h + self.h[0], c), data[b, m, h, c].item(), want[b, m, h, c].item()))
        rest = got.clone()
        self.lay.view(rest, "o", self.b, self.h, self.rows).fill_(CANARY)
        ne = rest != CANARY
        if ne.any():
            raise AssertionError("%s: %d elements of O the launch does not own changed (pad channels, rows behind Nq, gaps between "
                                 "items, other heads / rows / items of a sub-launch), first at buffer offset %d" % (
                                     what, ne.sum().item(), int(ne.nonzero()[0])))
        return err

    def same_bits(self, full, part, what=""):
        """The owned sub-range of `part` (this launch) against the same rows of `full` (the launch of everything), bit for bit."""
        a, b_ = self.lay.view(full.detach().cpu(), "o", self.b, self.h, self.rows), self.values(part)
        ne = a != b_
        if ne.any():
            b, m, h, c = (int(x) for x in ne.nonzero()[0])
            raise AssertionError("%s: %d elements of %d rows differ between the full launch and the sub-launch; first at %s: %r "
                                 "against %r" % (what, ne.sum().item(), ne.any(-1).sum().item(),
                                                 self.where(b + self.b[0], m + self.rows[0], h + self.h[0], c),
                                                 a[b, m, h, c].item(), b_[b, m, h, c].item()))


# ---- family A: selection.  K rows are +-1 codes, q_i = 64 k_t(i), t(i) = (a i + b0) mod Nk: with ATTN_INT_SCALE the selected
#      exponent argument is 8 D, every other one 8 dot(k_t, k_j)
ATTN_A_GAP = 40.0


def attn_select_nq(Nk):
    return Nk + ATTN_WG_ROWS + 5            # every key selected, from more than one wave; a ragged last workgroup


def make_attn_select(B, H, D, Nq, Nk, seed=1601):
    g = torch.Generator().manual_seed(seed + 7 * D + Nk)
    k = (torch.randint(0, 2, (B, Nk, H, D), generator=g) * 2 - 1).double()
    pool = torch.tensor([x for x in range(-100, 101) if x not in (0, 64, -64)], dtype=torch.float64)   # v and v + q never zero:
    v = pool[torch.randint(0, len(pool), (B, Nk, H, D), generator=g)]                                  # a relative bound means something
    a = next(x for x in (37, 29, 23, 19, 17, 13, 11, 7, 5, 3, 1) if x < max(Nk, 2) and math.gcd(x, Nk) == 1)
    i = torch.arange(Nq)
    sel = torch.stack([torch.stack([(a * i + 11 * b + 5 * h) % Nk for h in range(H)]) for b in range(B)])    # (B, H, Nq)
    q = torch.stack([torch.stack([64.0 * k[b, sel[b, h], h] for h in range(H)], 1) for b in range(B)])         # (B, Nq, H, D)
    return dict(q=q, k=k, v=v, sel=sel, a=a, scale=ATTN_INT_SCALE)


def attn_select_conditions(o):
    """Asserted on the CPU before any launch: every non-selected argument at least ATTN_A_GAP below the selected one, no two rows
    of V equal, every key selected, the selected argument 8 D.  -> the smallest gap"""
    q, k, v, sel = o["q"], o["k"], o["v"], o["sel"]
    B, Nk, H, D = k.shape
    assert attn_log2_scale(o["scale"]) == 0.125
    args = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.125
    top = args.gather(-1, sel[..., None])[..., 0]
    assert (top == 8 * D).all()
    rest = args.scatter(-1, sel[..., None], -1e9).max(-1).values
    gap = (top - rest).min().item() if Nk > 1 else float("inf")
    assert gap >= ATTN_A_GAP, "selection gap %g < %g" % (gap, ATTN_A_GAP)
    for b in range(B):
        for h in range(H):
            assert len({tuple(r.tolist()) for r in v[b, :, h]}) == Nk, "two rows of V are equal"
            assert len(set(sel[b, h].tolist())) == Nk, "a key is never selected"
            both = v[b, sel[b, h], h] + q[b, :, h]              # residual_q: integers of magnitude <= 164, bf16 values, never zero
            assert (both.abs() <= 164).all() and (both != 0).all() and (both.bfloat16().double() == both).all()
    assert (v != 0).all()
    return gap


# ---- family B: integer score levels.  k[:, 0] = 8 n_j, k[:, 1] = 8 u_j, q_i = (1, r_i, 0, ...): with ATTN_INT_SCALE the exponent
#      arguments are the integers n_j + r_i u_j; V holds integers in [1, 8]
ATTN_B_SCHEDULES = ("flat", "plus7", "plus8", "plus9", "falling", "saw", "one_lane")
ATTN_SAW = (0, 12, 3, 20, 5, 9, 30)


def attn_levels(schedule, nt):
    if schedule in ("flat", "one_lane"):
        return [40] * nt
    if schedule == "falling":
        return [100 - 9 * t for t in range(nt)]
    if schedule == "saw":
        return [40 + ATTN_SAW[t % len(ATTN_SAW)] + 40 * (t // len(ATTN_SAW)) for t in range(nt)]
    return [20 + {"plus7": 7, "plus8": 8, "plus9": 9}[schedule] * t for t in range(nt)]


def make_attn_levels(schedule, B, H, D, Nq, Nk, KT, seed=1701):
    g = torch.Generator().manual_seed(seed + Nk + D)
    nt = cdiv(Nk, KT)
    n = torch.empty(B, Nk, H, dtype=torch.float64)
    for t, lev in enumerate(attn_levels(schedule, nt)):
        lo, hi = t * KT, min((t + 1) * KT, Nk)
        n[:, lo:hi] = lev - torch.randint(1, 7, (B, hi - lo, H), generator=g).double()
        pos = torch.randint(0, hi - lo, (B, H), generator=g)                # the tile maximum at a drawn position
        for b in range(B):
            for h in range(H):
                n[b, lo + pos[b, h], h] = lev
    k = torch.zeros(B, Nk, H, D, dtype=torch.float64)
    q = torch.zeros(B, Nq, H, D, dtype=torch.float64)
    k[..., 0], q[..., 0] = 8 * n, 1.0
    if schedule == "one_lane":
        # one late key 5 above the flat level for everyone (no lane trips on it alone) and 10 above for the ONE query per wave
        # whose r is 1: that lane trips __any, its 31 neighbours advance by 5
        j = min(Nk - 1, (nt - 1) * KT + 2) if nt > 1 else Nk - 1
        k[:, j, :, 0] = 8 * (40 + 5)
        k[:, j, :, 1] = 8 * 5
        q[:, 13::ATTN_WAVE_ROWS, :, 1] = 1.0
    v = torch.randint(1, 9, (B, Nk, H, D), generator=g).double()
    return dict(q=q, k=k, v=v, scale=ATTN_INT_SCALE, schedule=schedule)


def attn_level_args(o, b=0, h=0):
    """the integer exponent arguments of one (batch, head), (Nq, Nk)"""
    a = (o["q"][b, :, h] @ o["k"][b, :, h].T) * 0.125
    assert (a == a.round()).all()
    return a


def attn_level_bound(dtype, Nk):
    """bf16: one bf16 ulp; fp32: the worst-case summation bound for positive terms, numerator and denominator"""
    return 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 * (Nk + 8) * 2.0 ** -24


# ---- family C: normal operands at three logit scales, judged per query row
ATTN_C_VARIANCES = (1, 4, 12)
ATTN_C_NK = {64: (65, 197, 485), 32: (33, 101, 243)}
ATTN_C_NQ = 165


def make_attn_float(B, H, D, Nq, Nk, variance, dtype, seed=1801):
    std = float(variance) ** 0.5
    f = std ** 0.5                          # q and k each by sqrt(std): the scores' standard deviation is std
    mk = lambda n, s, by: (randn((B, n, H, D), seed + s + Nk + D) * by).to(dtype).double()
    return dict(q=mk(Nq, 1, f), k=mk(Nk, 2, f), v=mk(Nk, 3, 1.0), scale=D ** -0.5, variance=variance)
