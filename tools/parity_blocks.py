"""Teacher-forced per-block bf16 parity at the FULL BASELINE.json geometries (run on the GPU box).

For every residual block / MultiScaleBlock of a workload (X3D-M 26, X3D-L 55, SlowFast-R50 16 + 16, MViT-B 16) plus its
stem and head:

    oracle block input (what the fp32 oracle feeds that block, rounded to bf16 -- the deploy form's storage type)
        -> the block ALONE in its bf16 deploy form (its own session, its own ingest: conv_a / conv_b / SE / conv_c /
           shortcut fusions exactly as inside the full plan)
        -> compared with the fp32 oracle's output of that block on the same input (fp32 weights, fp32 arithmetic)

Metric: max|d| / max|oracle block output|, bound 1e-2 (the north star's bf16 bar) per block.  No error of an earlier
block reaches a later one, so a kernel whose arithmetic moves shows up in exactly the blocks it serves -- the isolation
the chaotic end-to-end comparison cannot give (round-3 verdict, weak #3).  The token stream of MViT stays fp32 in the
deploy form, so its block inputs are handed over unrounded.

`batch` > 1: the library picks kernels by tile count, i.e. by batch, so the gate is run at the batch whose kernels it is
meant to judge.  `batch` distinct clips go through the fp32 oracle block by block; each block's deploy form is converted
for the `batch`-clip input and run once.  The metric is then taken per ROW (max|d| over the row / max|oracle block
output| over the same row; at batch 1 that is the metric above) and the block's figure is its worst row, whose index is
kept: a defect confined to the tail rows of a batch (a batch stride, a last partial tile) is named, not diluted.
`detail=True` additionally returns, per block,
  * the route: per op of the block's session the emitter's label, the op kind, the kernel symbol the library launched
    (Session.profile / op_kernels) and a geometry key (every scalar of the op's descriptor + which pointers are set), the
    same key the op has inside the full plan (`plan_route`);
  * the bf16-storage floor per row, from the reference side only: the same oracle block function under
    oracle.functional.storage_emulation on `quantize_like_kernels` weights against the fp32 oracle block output;
  * the sites that lie between the blocks in the full plan and were not part of the batch-1 gate (SlowFast's lateral
    fusions after res2 .. res4, MViT's patch embedding + position encoding, its final norm + head, and the norm1 operand a
    fused MLP writes for the next block), marked `extra`: with them every arithmetic op of the full plan has a counterpart
    here.  To have the same descriptors as in the full plan, the last slow-pathway block of a SlowFast stage writes into
    the channel slice of the wide (slow + lateral) buffer and an MViT block is emitted with its successor known.

    python tools/parity_blocks.py [--workloads x3d_m,x3d_l,slowfast_r50,mvit_b_32x3] [--fill trained_like] [--batch 1] [--json out.jsonl]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402


def _rel_rows(got, want):
    """Per batch row: max|d| over the row / max|want| over the same row."""
    d = (got.float().cpu() - want).abs().flatten(1).amax(1).tolist()
    n = want.abs().flatten(1).amax(1).tolist()
    return [a / max(b, 1e-12) for a, b in zip(d, n)]


def _q(t):
    return t.bfloat16().float()


# ------------------------------------------------------------------------------------------------ route
def geometry_key(fields):
    """Identifies a layer: every scalar (or list of scalars) of the op's descriptor by name -- batch, grid, channels, kernel,
    strides, leading dimensions, activation, dtype -- plus the names of the pointer fields that are set (residual, gate, second
    operand, ...).  Addresses themselves are left out: they differ between a block's own session and the full plan."""
    from pytorchvideo_amd.accelerator.mi355x.session import Ptr
    items = []
    for k in sorted(fields):
        v = fields[k]
        if v is None:
            continue
        if isinstance(v, Ptr):
            items.append("%s=*" % k)
        elif isinstance(v, (list, tuple)):
            items.append("%s=[%s]" % (k, ",".join("*" if isinstance(e, Ptr) else ("-" if e is None else repr(e)) for e in v)))
        else:
            items.append("%s=%r" % (k, v))
    return " ".join(items)


def session_route(sess, profile=True):
    """[{label, kind, kernel, geom}] per op of a finalized session that has run (`profile=False`: no device, kernel = None)."""
    if profile:
        sess.profile(iters=1)
    kernels = sess.op_kernels if profile else [None] * len(sess.ops)
    return [{"label": op[3], "kind": int(op[0]), "kernel": k, "geom": geometry_key(op[2])} for op, k in zip(sess.ops, kernels)]


# ------------------------------------------------------------------------------------------------ deploy units
def _read(sess, ref):
    if ref.T == ref.H == ref.W == 1 and ref.f32:
        return sess.view_rows(ref)[:, 0, :].float().cpu()           # logits
    if ref.thw is not None:
        return sess.view_rows(ref).float().cpu()                    # tokens (B, N, C)
    return sess.view(ref).float().cpu()


def _run_unit(emit, feeds, dry=False):
    """One stem / block / head / join alone in its own bf16 session: `emit(sess, input shapes) -> (input refs, output refs)`,
    feed the host tensors, launch once, read the outputs back (host fp32) and record the route."""
    from pytorchvideo_amd.accelerator.mi355x.session import Session
    sess = Session(dtype=torch.bfloat16)
    ins, outs = emit(sess, [tuple(t.shape) for t in feeds])
    if dry:
        return [None] * len(outs), session_route(sess, profile=False)
    sess.finalize()
    keep = []
    for t, ref in zip(feeds, ins):
        if ref.f32:
            sess.ingest_rows(t.cuda(), ref)                          # MViT's fp32 token stream
        else:
            d = t.cuda().to(torch.bfloat16)
            keep.append(d)                                           # a stem may read the clip itself: alive until the replay ran
            sess.feed(d, ref)
    sess.launch()
    got = [_read(sess, r) for r in outs]
    route = session_route(sess)
    del keep, sess
    return got, route


def _unit_single(module):
    """Stem / res block / head through its transmuter, as inside the full plan."""
    def emit(sess, shapes):
        from pytorchvideo_amd.accelerator.mi355x import blocks as B
        blk = B.transmute_single_io(copy.deepcopy(module))
        assert blk is not None, "block declined by the transmuter: %s" % type(module).__name__
        blk.convert(shapes[0], session=sess, dtype=torch.bfloat16)
        return [blk._in_ref], [blk._out_ref]
    return emit


def _unit_res_block_into_slice(c_extra):
    """The last slow-pathway block of a SlowFast stage: it stores into channels [0, C) of the buffer the lateral fusion
    completes (emit.emit_multipathway), so its output strides are those of the (C + c_extra)-wide buffer."""
    def make(module):
        def emit(sess, shapes):
            from pytorchvideo_amd.accelerator.mi355x import blocks as B
            from pytorchvideo_amd.accelerator.mi355x import emit as E
            blk = B.transmute_single_io(copy.deepcopy(module))
            assert blk is not None, "block declined by the transmuter: %s" % type(module).__name__
            Bn, Cc, T, H, W = shapes[0]
            x = sess.alloc_input(Bn, T, H, W, Cc)
            t_s, h_s, w_s, c_s = E.out_shape(blk, x)
            wide = sess.alloc_act(Bn, t_s, h_s, w_s, c_s + c_extra)
            out = wide.channel_slice(0, c_s)
            E.emit_module_out(sess, blk.eval(), x, out)
            return [x], [out]
        return emit
    return make


def _unit_lateral(fusion, c_slow):
    """FuseFastToSlow alone: conv (kt,1,1) stride (alpha,1,1) + BN + ReLU into channels [c_slow, c_slow + c_f) of the wide buffer."""
    def emit(sess, shapes):
        from pytorchvideo_amd.accelerator.mi355x import emit as E
        conv = copy.deepcopy(fusion.conv_fast_to_slow)
        Bn, Cc, T, H, W = shapes[0]
        fast = sess.alloc_input(Bn, T, H, W, Cc)
        To = E._conv_out(T, conv.kernel_size[0], conv.stride[0], E._triple(conv.padding)[0])
        wide = sess.alloc_act(Bn, To, H, W, c_slow + conv.out_channels)
        out = wide.channel_slice(c_slow, conv.out_channels)
        E.emit_lateral(sess, conv, fast, copy.deepcopy(fusion.norm).eval(), E.act_code(fusion.activation), out)
        return [fast], [out]
    return emit


def _unit_multipath(module):
    def emit(sess, shapes):
        from pytorchvideo_amd.accelerator.mi355x import blocks as B
        blk = B.transmute_multipath(copy.deepcopy(module))
        assert blk is not None, "container declined by the transmuter: %s" % type(module).__name__
        blk.convert(list(shapes), session=sess, dtype=torch.bfloat16)
        out = blk._out_ref
        return list(blk._in_ref), (list(out) if isinstance(out, list) else [out])
    return emit


def _unit_mvit_block(thw, nxt, seen):
    """A MultiScaleBlock with its successor known, as in the full plan: where the plan's fused MLP also writes norm1 of the
    next block (emit_mvit.emit_mlp_fused), so does this one, and that operand is the unit's second output."""
    def make(module):
        def emit(sess, shapes):
            from pytorchvideo_amd.accelerator.mi355x import blocks as B
            blk = B.Mi355xMViTBlock(copy.deepcopy(module))
            if nxt is not None:
                blk.__dict__["_pv_next_block"] = nxt
            try:
                blk.convert(shapes[0], session=sess, dtype=torch.bfloat16, thw=tuple(thw))
            finally:
                blk.__dict__.pop("_pv_next_block", None)
            out = blk._out_ref
            seen["thw"] = list(out.thw)
            outs = [out]
            if getattr(out, "prenorm", None) is not None:
                outs.append(out.prenorm[0])
            return [blk._in_ref], outs
        return emit
    return make


def _unit_mvit_prologue(model):
    def emit(sess, shapes):
        from pytorchvideo_amd.accelerator.mi355x import emit_mvit as EM
        Bn, Cc, T, H, W = shapes[0]
        x = sess.alloc_input(Bn, T, H, W, Cc)
        tok = EM.emit_patch_embed_and_pos(sess, copy.deepcopy(model.patch_embed).eval(),
                                          copy.deepcopy(model.cls_positional_encoding).eval(), x)
        return [x], [tok]
    return emit


def _unit_mvit_head(model, thw):
    def emit(sess, shapes):
        from pytorchvideo_amd.accelerator.mi355x import emit_mvit as EM
        Bn, N, Cc = shapes[0]
        x = sess.alloc_act(Bn, 1, 1, N, Cc, f32=True)
        x.thw, x.has_cls = tuple(thw), True
        return [x], [EM.emit_vit_head(sess, copy.deepcopy(model.norm_embed).eval(), copy.deepcopy(model.head).eval(), x)]
    return emit


# ------------------------------------------------------------------------------------------------ sites
# A site = one unit of the gate: {"names": one per output, "extra": not a row of the batch-1 gate, "module" / "make": the
# original-form module and how to turn (a copy of) it into a unit, "feeds": the oracle's inputs of the unit (host),
# "fn": (state dict, feeds) -> the oracle outputs, "wants": fn(sd, feeds)}.  The generators below walk the fp32 oracle's own
# trajectory: a unit's input never depends on what the deploy form produced.
def _site(names, make, module, feeds, fn, sd, extra=False, check=None):
    return {"names": names, "extra": extra, "make": make, "module": module, "feeds": feeds, "fn": fn, "wants": fn(sd, feeds),
            "check": check}


def _x3d_sites(m, sd, x, clip_len=16, crop=224):
    import math
    from oracle import functional as OF
    s0 = _site(["blocks.0 (stem)"], _unit_single, m.blocks[0], [_q(x)], lambda sd_, f: [OF.x3d_stem(sd_, f[0])], sd)
    yield s0
    h = s0["wants"][0]
    for s in range(1, 5):
        for i, rb in enumerate(m.blocks[s].res_blocks):
            p = "blocks.%d.res_blocks.%d" % (s, i)
            stride = (1, 2, 2) if i == 0 else (1, 1, 1)
            st = _site([p], _unit_single, rb, [_q(h)], lambda sd_, f, p=p, stride=stride: [OF.x3d_res_block(sd_, f[0], p, stride)], sd)
            yield st
            h = st["wants"][0]
    side = int(math.ceil(crop / 32))
    yield _site(["blocks.5 (head)"], _unit_single, m.blocks[5], [_q(h)],
                lambda sd_, f: [OF.x3d_head(sd_, f[0], "blocks.5", (clip_len, side, side))], sd)


def _slowfast_sites(m, sd, x):
    import torch.nn.functional as F
    from oracle import functional as OF

    def lateral(sd_, f, p):
        w = sd_[p + ".conv_fast_to_slow.weight"]
        z = F.conv3d(f, w, stride=(4, 1, 1), padding=(w.shape[2] // 2, 0, 0))
        return OF._st(torch.relu(OF._bn(z, sd_, p + ".norm")))

    def stems(sd_, f):
        s = OF.res_basic_stem(sd_, f[0], "blocks.0.multipathway_blocks.0")
        g = OF.res_basic_stem(sd_, f[1], "blocks.0.multipathway_blocks.1")
        return [torch.cat([s, lateral(sd_, g, "blocks.0.multipathway_fusion")], 1), g]

    # stems + first lateral fusion: the MultiPathWayWithFuse container as one unit
    s0 = _site(["blocks.0 (stems + fusion) slow", "blocks.0 (stems + fusion) fast"], _unit_multipath, m.blocks[0],
               [_q(x[0]), _q(x[1])], stems, sd)
    yield s0
    s, f = s0["wants"]
    del s0
    spatial = (1, 2, 2, 2)
    for st in range(4):
        fusion = m.blocks[st + 1].multipathway_fusion if st < 3 else None
        c_extra = fusion.conv_fast_to_slow.out_channels if fusion is not None else 0
        for pw in (0, 1):
            h = s if pw == 0 else f
            stage = m.blocks[st + 1].multipathway_blocks[pw]
            n = len(stage.res_blocks)
            for i, rb in enumerate(stage.res_blocks):
                p = "blocks.%d.multipathway_blocks.%d.res_blocks.%d" % (st + 1, pw, i)
                sb = (1, spatial[st], spatial[st]) if i == 0 else (1, 1, 1)
                make = _unit_res_block_into_slice(c_extra) if (pw == 0 and i == n - 1 and c_extra) else _unit_single
                site = _site([p], make, rb, [_q(h)], lambda sd_, t, p=p, sb=sb: [OF.bottleneck_res_block(sd_, t[0], p, (1, 1, 1), sb)], sd)
                yield site
                h = site["wants"][0]
                del site
            if pw == 0:
                s = h
            else:
                f = h
        if fusion is not None:
            # the lateral fusion site: its own unit (not a row of the batch-1 gate), and the teacher-forced trajectory goes on
            # from the fp32 oracle's concatenation
            p = "blocks.%d.multipathway_fusion" % (st + 1)
            site = _site([p + " (lateral)"], lambda fu, c=s.shape[1]: _unit_lateral(fu, c), fusion, [_q(f)],
                         lambda sd_, t, p=p: [lateral(sd_, t[0], p)], sd, extra=True)
            yield site
            del site
            s = torch.cat([s, lateral(sd, f, p)], 1)
    # PoolConcatPathway + head
    pool = _site(["blocks.5 (pool + concat)"], _unit_multipath, m.blocks[5], [_q(s), _q(f)],
                 lambda sd_, t: [OF._st(torch.cat([F.avg_pool3d(t[0], (8, 7, 7), stride=1), F.avg_pool3d(t[1], (32, 7, 7), stride=1)], 1))], sd)
    yield pool
    pooled = pool["wants"][0]
    yield _site(["blocks.6 (head)"], _unit_single, m.blocks[6], [_q(pooled)], lambda sd_, t: [OF.res_basic_head(sd_, t[0], "blocks.6")], sd)


def _mvit_sites(m, sd, x, cfg):
    import torch.nn.functional as F
    from oracle import functional as OF
    grid = {}

    def prologue(sd_, t):
        y = F.conv3d(t[0], sd_["patch_embed.patch_model.weight"], sd_.get("patch_embed.patch_model.bias"),
                     stride=cfg.get("conv_patch_embed_stride", (2, 4, 4)), padding=cfg.get("conv_patch_embed_padding", (1, 3, 3)))
        thw = [y.shape[2], y.shape[3], y.shape[4]]
        grid["thw"] = thw
        y = y.flatten(2).transpose(1, 2)
        c = "cls_positional_encoding"
        y = torch.cat((sd_[c + ".cls_token"].expand(y.shape[0], -1, -1), y), dim=1)
        pos = sd_[c + ".pos_embed_spatial"].repeat(1, thw[0], 1) + torch.repeat_interleave(sd_[c + ".pos_embed_temporal"], thw[1] * thw[2], dim=1)
        return [y + torch.cat([sd_[c + ".pos_embed_class"], pos], 1)]

    # the prologue (patch embedding with the position tables): its own unit, not a row of the batch-1 gate
    s0 = _site(["patch_embed + pos_encoding"], lambda mod: _unit_mvit_prologue(mod), m, [_q(x)], prologue, sd, extra=True)
    yield s0
    y, thw = s0["wants"][0], grid["thw"]
    del s0
    sched = OF.mvit_schedule(cfg)
    for i, (heads, kq, sq, kkv, skv) in enumerate(sched):
        nxt = m.blocks[i + 1] if i + 1 < len(sched) else None
        out = {}

        def block(sd_, t, i=i, thw=thw, a=(heads, kq, sq, kkv, skv), out=out, nxt=nxt):
            want, out["thw"] = OF.multiscale_block(sd_, t[0], thw, "blocks.%d" % i, a[0], a[1], a[2], a[3], a[4], True,
                                                   cfg.get("residual_pool", False), cfg.get("dim_mul_in_att", False))
            if nxt is None:
                return [want]
            return [want, OF._st(OF._block_norm(want, sd_, "blocks.%d.norm1" % (i + 1)))]

        seen = {}

        def check(seen=seen, out=out):
            assert list(seen["thw"]) == list(out["thw"]), (seen, out)

        site = _site(["blocks.%d" % i, "blocks.%d -> norm1 of blocks.%d" % (i, i + 1)], _unit_mvit_block(thw, nxt, seen), m.blocks[i], [y],
                     block, sd, check=check)
        site["extra_outputs"] = (1,)          # the second output is not a row of the batch-1 gate
        yield site
        y, thw = site["wants"][0], out["thw"]
        del site

    def head(sd_, t):
        return [F.linear(OF._st(OF._ln(t[0], sd_, "norm_embed"))[:, 0], sd_["head.proj.weight"], sd_["head.proj.bias"])]

    yield _site(["norm_embed + head"], lambda mod, thw=thw: _unit_mvit_head(mod, thw), m, [y], head, sd, extra=True)


def _sites(workload, m, sd, x):
    if workload in ("x3d_m", "x3d_l"):
        return _x3d_sites(m, sd, x)
    if workload == "slowfast_r50":
        return _slowfast_sites(m, sd, x)
    from pytorchvideo_amd.models.hub import mvit_video_base_32x3_config as cfg
    return _mvit_sites(m, sd, x, cfg)


def _floor_rows(site, sd_q, batch):
    """What bf16 storage ALONE does to this unit, per output and row: the oracle's own function under storage emulation on the
    kernels' weight rounding, against the fp32 oracle's output.  CPU only: no kernel of this repository takes part."""
    from oracle import functional as OF
    from pytorchvideo_amd.accelerator.mi355x import tuning       # the plan's own routing threshold, not a copy of it
    with OF.storage_emulation(torch.bfloat16, batch=batch, pool_stream_min_elems=tuning.get("pool_stream_min_elems")):
        emu = site["fn"](sd_q, site["feeds"])
    return [_rel_rows(e, w) for e, w in zip(emu, site["wants"])]


def _judge(site, emit, batch, sd_q=None, dry=False):
    """Run one site's unit; one record per output: {name, extra, rows, worst, worst_row, floor_rows, floor_worst, route}."""
    got, route = _run_unit(emit, site["feeds"], dry=dry)
    if site["check"] is not None:
        site["check"]()
    floors = _floor_rows(site, sd_q, batch) if sd_q is not None else None
    recs = []
    for j, g in enumerate(got):
        rows = _rel_rows(g, site["wants"][j]) if g is not None else []
        worst_row = max(range(len(rows)), key=lambda r: rows[r]) if rows else None
        rec = {"name": site["names"][j], "extra": bool(site["extra"] or j in site.get("extra_outputs", ())), "rows": rows,
               "worst": rows[worst_row] if rows else None, "worst_row": worst_row, "route": route if j == 0 else []}
        if floors is not None:
            rec["floor_rows"] = floors[j]
            rec["floor_worst"] = max(floors[j])
        recs.append(rec)
    return recs


def blocks_case(workload, fill="trained_like", batch=1, detail=False, floor=None, dry=False):
    """[(block name, max|d| / max|oracle block output|)] for every block of `workload` at its BASELINE geometry; with `batch`
    clips the figure is that of the block's worst row.  `detail=True`: a list of records instead (see the module docstring)
    that also holds the `extra` sites; `floor` (default: with `detail`) adds the reference-only bf16-storage floor per row;
    `dry=True` emits every unit without a device (routes carry labels and geometry keys, no kernel symbols, no figures)."""
    from bench import synth_input
    from oracle.weights import quantize_like_kernels
    from parity_full import filled_model
    m, shape = filled_model(workload, fill)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = synth_input(shape, batch, 99)
    floor = detail if floor is None else floor
    sd_q = quantize_like_kernels(sd) if (floor and not dry) else None
    recs = []
    with torch.no_grad():
        for site in _sites(workload, m, sd, x):
            recs += _judge(site, site["make"](site["module"]), batch, sd_q, dry)
            del site                                    # a block's tensors go before the next block's are made
    if not dry:
        torch.cuda.empty_cache()
    if detail:
        return recs
    return [(r["name"], r["worst"]) for r in recs if not r["extra"]]


def plan_route(workload, fill="trained_like", batch=None, streams=None):
    """The route of the bench form's sub-plan 0: the deploy form built as bench.py builds it (same weights, per-GPU batch,
    `streams` sub-batch plans), run once, then profiled.  Same record per op as `blocks_case(..., detail=True)` keeps."""
    from bench import WORKLOADS, synth_input
    from parity_full import filled_model
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    batch = WORKLOADS[workload]["batch"] if batch is None else batch
    streams = WORKLOADS[workload].get("streams", 1) if streams is None else streams
    m, shape = filled_model(workload, fill)
    x = synth_input(shape, batch, 99)
    transmute_model(m, "mi355x")
    xd = [t.cuda().bfloat16() for t in x] if isinstance(x, list) else x.cuda().bfloat16()
    dm = convert_to_deployable_form(m, xd, dtype=torch.bfloat16, streams=streams)
    dm(list(xd) if isinstance(xd, list) else xd)
    torch.cuda.synchronize()
    route = session_route(dm._pv_session)
    torch.cuda.synchronize()
    del dm
    torch.cuda.empty_cache()
    return route


def defect_case(workload, block, scale=1.05, fills=("calibrated", "trained_like"), batch=1, conv="conv_c"):
    """Defect injection: `block` = "blocks.S.res_blocks.I" of an X3D model or
    "blocks.S.multipathway_blocks.P.res_blocks.I" of SlowFast, teacher-forced at `batch` clips; the deploy form is built twice --
    as is, and with the filter bank of the block's `conv` (conv_a / conv_b / conv_c) scaled by `scale` (a 5 % arithmetic defect
    in one kernel's operand) -- and both are compared with the fp32 oracle's output of the UNTOUCHED block, per row, worst row
    reported.  {fill: {"clean": e, "defect": e, "clean_row": r, "defect_row": r, "route": the clean unit's route}}."""
    assert workload in ("x3d_m", "x3d_l", "slowfast_r50")
    from bench import synth_input
    from parity_full import filled_model
    out = {"workload": workload, "block": block, "scale": scale, "batch": batch, "conv": conv}
    for fill in fills:
        m, shape = filled_model(workload, fill)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        x = synth_input(shape, batch, 99)
        with torch.no_grad():
            for site in _sites(workload, m, sd, x):
                if site["names"][0] == block:
                    break
                del site
            else:
                raise KeyError(block)
            clean = _judge(site, site["make"](site["module"]), batch)[0]
            bad = copy.deepcopy(site["module"])
            getattr(bad.branch2, conv).weight.mul_(scale)
            defect = _judge(site, site["make"](bad), batch)[0]
            del site
        out[fill] = {"clean": clean["worst"], "defect": defect["worst"], "clean_row": clean["worst_row"],
                     "defect_row": defect["worst_row"], "route": clean["route"]}
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="x3d_m,x3d_l,slowfast_r50,mvit_b_32x3")
    ap.add_argument("--fill", default="trained_like")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    for w in a.workloads.split(","):
        rows = blocks_case(w, a.fill, batch=a.batch)
        worst = max(rows, key=lambda r: r[1])
        rec = {"workload": w, "fill": a.fill, "blocks": len(rows), "worst": worst[1], "worst_block": worst[0],
               "per_block": {k: float("%.3e" % v) for k, v in rows}}
        if a.batch != 1:
            rec["batch"] = a.batch
        print(json.dumps(rec), flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(json.dumps(rec) + "\n")
