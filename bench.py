"""Forward-throughput benchmark of the MI355X path (clips/s), one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload x3d_m|x3d_l|slowfast_r50|mvit_b_32x3]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one forward of the hot path over one batch of synthetic clips that is already
resident in HBM in the reference's own layout ([B,3,T,H,W], bf16); every rank processes a
fixed per-GPU batch (weak scaling) and the step ends with the single head collective
(all_gather of the [B_local, 400] fp32 logits).  Rank 0 prints ONE JSON line.

`--gpus N` without a torchrun environment (WORLD_SIZE unset) re-executes this file under
`torch.distributed.run` with N ranks on 127.0.0.1, so `python bench.py --gpus 8` is the same
job as the explicit launcher line above.

Default workload = BASELINE.json configs[1]: X3D-M, bf16, [32,3,16,224,224] per GPU.  A plain run (no --full) builds
the workload, runs W warm-up steps and K timed steps and prints the line.

`--full` adds everything else the line can carry: a >= 2 s sustained run, the roofline object (per-op profiling of the
single-plan form), the CPU baseline at N = 1 and, under "secondary", MViT-B 32x3 (configs[3], the other model
BASELINE.json's metric names), SlowFast-R50 8x8 (configs[2]) and X3D-L (configs[4]) -- each with its own step
percentiles, sustained run and roofline object.  At N > 1 the secondary legs are MViT-B (the metric names it at
1/2/4/8 GPUs) and X3D-L (configs[4]: global batch 32 N sharded over the N GPUs).  The --no-* options drop single parts
of a --full run.

`--dump-outputs DIR` writes what the last timed step returned, the [global batch, 400] logits, to DIR/logits.npy
(float32).  Weights and inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import re
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_PEAK_TFS = 2500.0    # dense bf16
VALU_PEAK_TFS = 157.3     # fp32 vector pipe (packed FMA), MI355X_MICROARCH.md
VALU_BOUND_SYMBOLS = ("pwdw_plane_kernel", "dw3_plane_kernel", "dwconv_kernel", "bottleneck_block_kernel")   # fp32 depthwise stencils

# algorithmic FLOPs / bytes per clip (probe of the reference op graph)
WORKLOADS = {
    "x3d_m": dict(batch=32, gflop=9.465, mb=365.0, bound="hbm", streams=2,
                  desc="create_x3d(input_clip_length=16,input_crop_size=224) [B,3,16,224,224]"),
    "x3d_l": dict(batch=32, gflop=18.325, mb=604.0, bound="hbm", streams=2,
                  desc="create_x3d(16,224,depth_factor=5.0) [B,3,16,224,224]"),
    # (two branches since round 6: 2673 -> 2716 clips/s over three interleaved pairs, profiles/r6/model_ab_slowfast_streams_call90.txt;
    #  rounds 2-5 measured +-0 and kept one plan)
    "slowfast_r50": dict(batch=16, gflop=131.42, mb=740.0, bound="mfma", streams=2,
                         desc="create_slowfast(model_depth=50) slow [B,3,8,256,256] + fast [B,3,32,256,256]"),
    "mvit_b_32x3": dict(batch=8, gflop=339.92, mb=1465.0, bound="mfma", streams=2,
                        desc="create_multiscale_vision_transformers(**mvit_video_base_32x3_config) [B,3,32,224,224]"),
    # launcher check only (tests/test_bench_launcher.py): tiny clip, original-form model on the host, gloo
    "x3d_xs_dry": dict(batch=2, gflop=1.211, mb=0.0, bound="hbm",
                       desc="create_x3d(input_clip_length=4,input_crop_size=160) [B,3,4,160,160]"),
}


def make_model(name):
    """(original-form model, input shape(s)) of a workload."""
    if name in ("x3d_m", "x3d_l", "x3d_xs_dry"):
        from pytorchvideo_amd.models import create_x3d
        kw = dict(input_clip_length=16, input_crop_size=224)
        if name == "x3d_l":
            kw["depth_factor"] = 5.0
        if name == "x3d_xs_dry":
            kw = dict(input_clip_length=4, input_crop_size=160)
        return create_x3d(**kw), (3, kw["input_clip_length"], kw["input_crop_size"], kw["input_crop_size"])
    if name == "slowfast_r50":
        from pytorchvideo_amd.models import create_slowfast
        return create_slowfast(model_depth=50), [(3, 8, 256, 256), (3, 32, 256, 256)]
    if name == "mvit_b_32x3":
        from pytorchvideo_amd.models import create_multiscale_vision_transformers
        from pytorchvideo_amd.models.hub import mvit_video_base_32x3_config as cfg
        return create_multiscale_vision_transformers(**cfg), (3, 32, 224, 224)
    raise SystemExit("unknown workload %s" % name)


def oracle_forward(name):
    """CPU oracle of a workload: ONLY the cpu_baseline leg calls this (oracle/ is test infrastructure)."""
    from oracle import functional as OF
    if name in ("x3d_m", "x3d_l"):
        return lambda sd, x: OF.x3d_forward(sd, x, 16, 224)
    if name == "slowfast_r50":
        return lambda sd, x: OF.slowfast_forward(sd, x[0], x[1])
    from pytorchvideo_amd.models.hub import mvit_video_base_32x3_config as cfg
    return lambda sd, x: OF.mvit_forward(sd, x, cfg)


def synth_input(shape, batch, seed):
    """Synthetic clips; SlowFast's slow pathway is the temporally subsampled fast pathway
    (PackPathway: uniform_temporal_subsample, transforms/functional.py:134-160)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    if isinstance(shape, list):
        fast = torch.randn((batch,) + tuple(shape[1]), generator=g)
        idx = torch.linspace(0, shape[1][1] - 1, shape[0][1]).long()
        return [fast[:, :, idx].contiguous(), fast]
    return torch.randn((batch,) + tuple(shape), generator=g)


_WEIGHTS = {}


def build_model(name, batch, device, dtype, streams=1):
    import torch
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.utils import synthetic_trained_like_weights
    torch.manual_seed(0)
    model, shape = make_model(name)
    # the instance tests/test_gpu_full_geometry.py checks against the fp32 oracle at this batch and stream count
    # (oracle.weights.trained_like_fill draws the same values: tests/test_host.py pins the two fills to each other)
    if name in _WEIGHTS:       # (the roofline pass rebuilds the single-plan form: calibrate on the host once per workload)
        model.load_state_dict(_WEIGHTS[name])
        model.eval()
    else:
        synthetic_trained_like_weights(model, synth_input(shape, 2, 7), 0)
        _WEIGHTS[name] = {k: v.clone() for k, v in model.state_dict().items()}
    x = synth_input(shape, batch, 1234 + int(os.environ.get("RANK", "0")))
    x = [t.to(dtype).to(device) for t in x] if isinstance(x, list) else x.to(dtype).to(device)
    transmute_model(model, "mi355x")
    deployed = convert_to_deployable_form(model, x, dtype=dtype, streams=streams)
    return deployed, x


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _reference_model(name):
    """The REAL reference model of a workload (facebookresearch/pytorchvideo under PV_REFERENCE_ROOT, imported through
    oracle/ref_shim.py) or None where the reference tree does not exist (the GPU box)."""
    root = os.environ.get("PV_REFERENCE_ROOT", "/root/reference")
    if not os.path.isdir(os.path.join(root, "pytorchvideo")):
        return None
    try:
        from oracle import ref_shim
        ref_shim.install()
        if name in ("x3d_m", "x3d_l"):
            from pytorchvideo.models.x3d import create_x3d as ref_create_x3d
            kw = dict(input_clip_length=16, input_crop_size=224)
            if name == "x3d_l":
                kw["depth_factor"] = 5.0
            return ref_create_x3d(**kw)
        if name == "slowfast_r50":
            from pytorchvideo.models.slowfast import create_slowfast as ref_create_slowfast
            return ref_create_slowfast(model_depth=50)
        from pytorchvideo.models.hub.vision_transformers import mvit_video_base_32x3_config as cfg
        from pytorchvideo.models.vision_transformers import create_multiscale_vision_transformers as ref_create_mvit
        return ref_create_mvit(**cfg)
    except Exception as e:       # an incomplete tree: fall back to the port, and say so
        print("cpu_baseline: reference not importable (%s); timing the oracle port" % e, file=sys.stderr)
        return None


def cpu_baseline(name):
    """The reference's own CPU forward timed on this box's host cores when the reference tree is present
    (kind "reference": the real pytorchvideo modules, fp32, eval, no_grad), else the oracle (kind "port":
    oracle/functional.py, the reference forward restated op for op on torch-CPU, pinned bit-exact to the reference by
    tests/golden).  Bounded sample of the same workload: 8 clips (X3D; 4 / 2 for SlowFast / MViT), per thread count 1 warm-up
    + 3 timed iterations, best kept; thread counts {4, 8, 16, 32} capped by the host (round 6: round 5's {8, 16, 32, 64} again had its
    optimum on the lower edge; round 4's {32, 64, 128} sweep was monotonically DEcreasing on the 256-thread box) and the spread of
    the sweep is part of the record.  Baseline, not target."""
    import torch
    from oracle.weights import reference_style_fill
    nproc = os.cpu_count() or 1
    b = {"x3d_m": 8, "x3d_l": 8, "slowfast_r50": 4, "mvit_b_32x3": 2}[name]
    _, shape = make_model(name)
    x = synth_input(shape, b, 7)
    ref = _reference_model(name)
    if ref is not None:
        reference_style_fill(ref, 0).eval()
        fwd, kind = (lambda: ref(list(x) if isinstance(x, list) else x)), "reference"
        what = "the reference's own modules (pytorchvideo.models via oracle/ref_shim.py)"
    else:
        m, _ = make_model(name)
        reference_style_fill(m, 0).eval()
        sd, oracle_fn = m.state_dict(), oracle_forward(name)
        fwd, kind = (lambda: oracle_fn(sd, x)), "port"
        what = ("torch-CPU oracle (oracle/functional.py, op-for-op restatement of the reference, bit-exact vs the "
                "reference fixtures; /root/reference does not exist on this box)")
    sweep, t_budget = {}, time.perf_counter()
    spread = {}
    for cores in sorted({min(nproc, c) for c in (8, 16, 4, 32)}, key=lambda c: (c != 8, c != 16, c)):   # 8 and 16 first: the optimum of rounds 4-5 sat at the sweep's lower edge
        torch.set_num_threads(cores)
        with torch.no_grad():
            fwd()   # warm-up (oneDNN primitive creation, allocator)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                fwd()
                ts.append(time.perf_counter() - t0)
        sweep[cores] = round(b / min(ts), 3)
        spread[cores] = round(max(ts) / min(ts), 3)
        if time.perf_counter() - t_budget > 45.0:      # bounded: the default bench line must finish within minutes
            break
    cores = max(sweep, key=sweep.get)
    return {"value": sweep[cores], "unit": "clips/s", "cores": cores, "kind": kind, "cpu": cpu_model_name(), "nproc": nproc,
            "threads_sweep": {str(k): v for k, v in sorted(sweep.items())},
            "sweep_spread": {"min": min(sweep.values()), "max": max(sweep.values()),
                             "note": "driver-run values of rounds 1-5 on other boxes / samplings: 3.9 / 6.3 / 8.7 / 7.3 / 3.9 clips/s"} if name == "x3d_m" else
                            {"min": min(sweep.values()), "max": max(sweep.values())},
            "slowest_over_fastest_iteration": {str(k): v for k, v in sorted(spread.items())},
            "sample": "%d clips, fp32, %s, 1 warm-up + 3 timed per thread count, best of the sweep" % (b, what)}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_spawn(args):
    """`python bench.py --gpus N` outside a torchrun environment: become the launcher."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.call(cmd, env=env)


def roofline_session(model, name, batch, device, args):
    """The plan whose kernels the `roofline` object describes: the full per-GPU batch as ONE plan, every kernel
    alone on the chip (what `rocprofv3 --kernel-trace -- python bench.py --streams 1` sees).  With streams > 1 the
    timed steps overlap kernels of different sub-batches, where a per-kernel duration is not defined; the
    per-kernel evidence is therefore taken from the single-plan form of the same batch."""
    if not hasattr(model, "parts"):
        return model._pv_session
    import torch
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    single, x = build_model(name, batch, device, dtype, streams=1)
    for _ in range(2):
        single(list(x) if isinstance(x, list) else x)
    torch.cuda.synchronize()
    roofline_session.keep = (single, x)      # alive while its session is profiled
    return single._pv_session


def roofline_of(sess, workload, clips_s_per_gpu, ms_per_step):
    """Per-op device time measured live (pv_plan_profile: in-situ HIP events on the launch stream, host kept out of
    the measurement), folded per KERNEL SYMBOL (pv_plan_op_kernel: the kernel each op was routed to); the dominant
    kernel's algorithmic rate against its roofline.  Returns (roofline dict, per-op list, per-label dict)."""
    wl = WORKLOADS[workload]
    prof = sess.profile(iters=3)
    kernels = getattr(sess, "op_kernels", None) or [""] * len(prof)
    agg, by_kernel = {}, {}
    for (label, kind, ms, alg_bytes, flops), sym in zip(prof, kernels):
        label = label.split("|")[0]
        fam = label.split(".")[0] if label.startswith(("conv_b", "conv_ab")) else label
        for table, key in ((agg, fam), (by_kernel, sym or fam)):
            a = table.setdefault(key, [0, 0.0, 0, 0, {}])
            a[0] += 1
            a[1] += ms
            a[2] += alg_bytes
            a[3] += flops
            a[4][fam] = a[4].get(fam, 0.0) + ms
    total_kernel_ms = sum(v[1] for v in agg.values())
    dom_sym, dom = max(by_kernel.items(), key=lambda kv: kv[1][1])
    # the dominant kernel's roofline: HBM when its arithmetic intensity is below the ridge
    # (2.5 PFLOP/s / 8 TB/s = 312 FLOP/B), MFMA otherwise
    dom_gbs = dom[2] / (dom[1] * 1e-3) / 1e9 if dom[1] > 0 else 0.0
    dom_tfs = dom[3] / (dom[1] * 1e-3) / 1e12 if dom[1] > 0 else 0.0
    mfma_bound = dom[2] > 0 and dom[3] / dom[2] > MFMA_PEAK_TFS * 1e12 / (HBM_PEAK_GBS * 1e9)
    # HBM traffic of that kernel from the rocprofv3 PMC passes of the SAME code (tools/gpu_evidence.sh +
    # tools/summarize_pmc.py -> profiles/traffic.json, stamped with the commit it was measured on), else null
    # Looked up by KERNEL SYMBOL (the "_by_kernel" table: every dispatch of that symbol in the PMC passes, i.e. the
    # same population `alg_bytes_per_launch` averages over); where only per-op-label figures exist, each of the
    # symbol's ops takes its label's figure and `traffic_population` says so.
    traffic = traffic_commit = traffic_pop = None
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        ent = tj.get(workload, {})
        sym_ent = (ent.get("_by_kernel") or {}).get(dom_sym)
        if sym_ent:
            traffic = sym_ent.get("hbm_bytes_per_launch")
            traffic_pop = "every dispatch of the symbol in the PMC passes (%d profiled)" % sym_ent.get("dispatches_profiled", 0)
        else:
            n_by_label = {}
            for (label, kind, ms, alg_bytes, flops), sym in zip(prof, kernels):
                if (sym or "") == dom_sym:
                    lab = label.split("|")[0]
                    lab = lab.split(".")[0] if lab.startswith(("conv_b", "conv_ab")) else lab
                    n_by_label[lab] = n_by_label.get(lab, 0) + 1
            known = {k: ent[k]["hbm_bytes_per_launch"] for k in n_by_label if k in ent}
            if known and len(known) == len(n_by_label):
                traffic = int(sum(known[k] * n_by_label[k] for k in known) / sum(n_by_label.values()))
                traffic_pop = "per-op-label PMC figures weighted by this symbol's ops: " + ", ".join(
                    "%s x%d" % kv for kv in sorted(n_by_label.items()))
        traffic_commit = tj.get("_measured_on", {}).get(workload)
    except (OSError, ValueError, KeyError):
        pass
    plan_bytes = sum(p[3] for p in prof)          # the plan's OWN algorithmic bytes per step (after its fusions)
    # A depthwise-stencil symbol is bound by the fp32 VECTOR pipe, not by HBM (75-78 % VALU busy, ~1.6x above the
    # stencil's own issue cycles): report that roof beside the byte roof.  Its stencil FLOPs are 2 x 27 taps per output value
    # = the op's FLOPs minus the fused pointwise producer's (emit.py counts both); the fp32 peak is the packed-FMA rate.
    def stencil_flops(label, flops):
        """fp32 FMAs x 2 of the 3-D stencil inside an op (its fused pointwise convs excluded), from the op label."""
        m2 = re.search(r"\|(\d+)x(\d+)x(\d+)x(\d+) c(\d+)", label)
        m = re.search(r"c(\d+)->(\d+)(?:->\d+)? k1x1x1\+k(\d)x(\d)x(\d)", label)   # conv_ab / block.fused: producer cin -> C [-> cout], then the stencil
        if m and m2:
            B_, T_, H_, W_ = (int(v) for v in m2.groups()[:4])
            return 2 * B_ * T_ * H_ * W_ * int(m.group(2)) * int(m.group(3)) * int(m.group(4)) * int(m.group(5))
        return flops

    valu_by_sym = {}
    for (label, kind, ms, alg_bytes, flops), sym in zip(prof, kernels):
        if (sym or "") in VALU_BOUND_SYMBOLS:
            e = valu_by_sym.setdefault(sym, [0.0, 0.0])
            e[0] += stencil_flops(label, flops)
            e[1] += ms
    second_roofs = {}
    for sym, (fl, ms) in valu_by_sym.items():
        if fl and ms > 0:
            tf = fl / (ms * 1e-3) / 1e12
            second_roofs[sym] = {"bound": "valu", "achieved": round(tf, 2), "peak": VALU_PEAK_TFS, "unit": "TFLOP/s (fp32 stencil FMAs)",
                                 "frac": round(tf / VALU_PEAK_TFS, 4), "kernel_ms_per_step": round(ms, 4)}
    valu = second_roofs.get(dom_sym)
    r = {
        "bound": "mfma" if mfma_bound else "hbm", "kernel": dom_sym, "launches_per_step": dom[0],
        "op_labels": {k: round(v, 4) for k, v in sorted(dom[4].items(), key=lambda kv: -kv[1])},
        "achieved": round(dom_tfs if mfma_bound else dom_gbs, 1),
        "peak": MFMA_PEAK_TFS if mfma_bound else HBM_PEAK_GBS, "unit": "TFLOP/s" if mfma_bound else "GB/s",
        "frac": round(dom_tfs / MFMA_PEAK_TFS if mfma_bound else dom_gbs / HBM_PEAK_GBS, 4),
        "traffic": traffic, "traffic_measured_on": traffic_commit, "traffic_population": traffic_pop,
        "alg_bytes_per_launch": int(dom[2] / max(dom[0], 1)), "alg_flops_per_launch": int(dom[3] / max(dom[0], 1)),
        "avg_launch_ms": round(dom[1] / max(dom[0], 1), 5),
        "kernel_ms_per_step": round(dom[1], 4), "all_kernels_ms_per_step": round(total_kernel_ms, 4),
        "launches_total": len(prof),
        "kernels_ms_per_step": {k: round(v[1], 4) for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1][1])[:6]},
        "timing": "pv_plan_profile on the single-plan form of the per-GPU batch (every kernel alone on the chip, = "
                  "bench.py --streams 1): each op timed in situ between its own HIP event pair behind a queued replay, "
                  "min of 3, null event interval subtracted; ops folded by the kernel symbol they were routed to",
        # whole model against the HBM roofline, two byte models: SURVEY 8d's per-op model of the REFERENCE op graph
        # (each Conv/Linear reads its input and writes its output once; wl['mb'] MB per clip) and this plan's own
        # algorithmic bytes (what its fused kernels have to move: fewer bytes, so a lower -- stricter -- fraction)
        "model_hbm_frac": round(clips_s_per_gpu * wl["mb"] * 1e6 / (HBM_PEAK_GBS * 1e9), 4),
        "model_hbm_frac_plan": round(plan_bytes / max(ms_per_step, 1e-9) / 1e6 / HBM_PEAK_GBS, 4),
        "plan_alg_mb_per_step": round(plan_bytes / 1e6, 1),
        "model_mfma_frac": round(clips_s_per_gpu * wl["gflop"] * 1e9 / (MFMA_PEAK_TFS * 1e12), 4),
    }
    if valu is not None:
        r["second_roof"] = {k: v for k, v in valu.items() if k != "kernel_ms_per_step"}      # the symbol against BOTH roofs (round-4 verdict, weak #11)
    if second_roofs:
        r["second_roofs"] = second_roofs      # ... and every fp32-stencil symbol of the step, dominant or not (round-5 verdict, item 7)
    return r, prof, agg


def timed_steps(step, steps, world, device):
    """EXACTLY `steps` steps between barrier + synchronize on both sides; max over ranks."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    out = None
    for i in range(steps):
        out = step()
        marks[i + 1].record()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    return elapsed, step_ms, out


def run_workload(name, args, world, rank, device, steps, warmup, sustained_s=0.0, prewarm_s=0.0):
    """Build, warm up, time; returns (result dict, deployed model, input, step, host copy of the last timed step's output,
    taken before the sustained run replays the step again).  prewarm_s (secondary legs only): untimed replays
    for that long BEFORE the W warm-up steps -- the host-side conversion of a leg's model leaves the GPU idle for seconds,
    and twice in three default runs the X3D-L leg (the longest conversion, the last leg) had one or two ~25 ms replays
    among its first timed steps behind 5 warm-up replays (p50 5.4 ms; profiles/r6/bench_default_line.json of calls 83 / 91)."""
    import torch
    from pytorchvideo_amd.parallel import gather_logits
    wl = WORKLOADS[name]
    batch = args.batch or wl["batch"]
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    streams = args.streams if args.streams > 0 else wl.get("streams", 1)
    model, x = build_model(name, batch, device, dtype, streams=streams)
    if args.no_graph:
        for part in getattr(model, "parts", [model]):
            part.__dict__["_pv_use_graph"] = False

    comm = None if args.no_graph else HEAD["comm"]      # pv_forward_gather replays a graph
    if comm is not None:
        # the step is ONE C call behind the input ingest: graph replay, logits rows of the sub-plans, ncclAllGather
        # enqueued by the library itself on the launch stream (pv_forward_gather, include/pv_mi355x.h)
        from pytorchvideo_amd.parallel import ShardedForward
        sharded = ShardedForward(model, comm)

        def step():
            return sharded(list(x) if isinstance(x, list) else x)

        if world > 1:     # once per workload: the C-driven collective against torch.distributed's on the same logits
            ref = gather_logits(model(list(x) if isinstance(x, list) else x), global_batch=batch * world)
            got = step()
            torch.cuda.synchronize()
            if not torch.equal(got, ref):
                raise SystemExit("pv_forward_gather disagrees with torch.distributed's all_gather on rank %d" % rank)
    else:
        def step():
            return gather_logits(model(list(x) if isinstance(x, list) else x), global_batch=batch * world)

    if prewarm_s > 0:
        t_pre = time.perf_counter()
        while time.perf_counter() - t_pre < prewarm_s:
            out = step()
            torch.cuda.synchronize()
    for _ in range(warmup):
        out = step()
    elapsed, step_ms, out = timed_steps(step, steps, world, device)
    assert out.shape == (batch * world, 400) and torch.isfinite(out).all()
    last = out.detach().float().cpu()
    pct = lambda q: round(step_ms[min(len(step_ms) - 1, int(q * len(step_ms)))], 4)
    res = {"value": round(batch * world * steps / elapsed, 2), "ms_per_step": round(elapsed / steps * 1e3, 4),
           "step_ms": {"p10": pct(0.1), "p50": pct(0.5), "p90": pct(0.9)}, "steps": steps, "per_gpu_batch": batch,
           "streams": len(getattr(model, "parts", [0]))}
    if sustained_s > 0:   # a run long enough for clocks / power to settle: same step, >= sustained_s seconds
        n = max(steps, int(sustained_s / max(elapsed / steps, 1e-6)) + 1)
        e2, _, _ = timed_steps(step, n, world, device)
        res["sustained"] = {"seconds": round(e2, 3), "steps": n, "value": round(batch * world * n / e2, 2),
                            "ms_per_step": round(e2 / n * 1e3, 4)}
    return res, model, x, step, last


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each host tensor of `arrays` as out_dir/<name>.npy in float32.  The logits are 1.6 KB per clip, so
    the whole output always fits the limit at any batch a GPU holds; a larger dump is refused rather than sampled."""
    import numpy as np
    total = sum(t.numel() * 4 for t in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


# the head collective of this process: a pv_comm communicator (RCCL driven from C) at N > 1 or with --head-comm
HEAD = {"comm": None, "how": "none (one rank: the logits stay where they are)"}


def setup_head_collective(args, world):
    """N > 1 (or --head-comm at N = 1): bind RCCL inside the C library and create the communicator; every step then
    calls pv_forward_gather.  If no rank-wide binding is possible the step falls back to torch.distributed's
    all_gather_into_tensor (the same RCCL, called from Python) and the line says so."""
    if world == 1 and not args.head_comm:
        return
    try:
        from pytorchvideo_amd.parallel import HeadComm
        HEAD["comm"] = HeadComm()
        HEAD["how"] = ("pv_forward_gather: graph launch + ncclAllGather enqueued from C on the launch stream (pv_comm over %s)"
                       % HEAD["comm"].library)
    except Exception as e:      # noqa: BLE001 -- any failure to bind: report it, keep the torch.distributed route
        if args.head_comm == "require":
            raise
        HEAD["how"] = "torch.distributed all_gather_into_tensor from Python (pv_comm unavailable: %s)" % str(e)[:200]


def pcie_leg(model, x, step, batch, steps, device):
    """The same steps with the host -> device upload of the batch inside the timed region (never `value`)."""
    import torch
    xs = x if isinstance(x, list) else [x]
    hs = [t.cpu().pin_memory() for t in xs]
    for _ in range(2):
        for t, h in zip(xs, hs):
            t.copy_(h, non_blocking=True)
        step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(steps):
        for t, h in zip(xs, hs):
            t.copy_(h, non_blocking=True)
        step()
    torch.cuda.synchronize()
    e1 = time.perf_counter() - t1
    pcie = {"value": round(batch * steps / e1, 2), "unit": "clips/s (this rank)", "ms_per_step": round(e1 / steps * 1e3, 4),
            "upload_bytes_per_step": int(sum(h.numel() * h.element_size() for h in hs))}
    # ... and with the pre-path transforms fused into the ingest (pytorchvideo_amd.transforms.DevicePacker): one uint8
    # clip at the fast frame rate is uploaded, every pathway is subsampled / scaled / normalised on the device
    from pytorchvideo_amd.transforms import DevicePacker
    ratios = (xs[-1].shape[2] // xs[0].shape[2], 1) if len(xs) == 2 else None
    packer = DevicePacker(model, (0.45,) * 3, (0.225,) * 3, div255=True, frame_ratios=ratios)
    u8 = torch.randint(0, 256, tuple(xs[-1].shape), dtype=torch.uint8).pin_memory()
    d8 = torch.empty_like(u8, device=device)
    for _ in range(2):
        d8.copy_(u8, non_blocking=True)
        packer(d8)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for _ in range(steps):
        d8.copy_(u8, non_blocking=True)
        packer(d8)
    torch.cuda.synchronize()
    e2 = time.perf_counter() - t2
    pcie["u8_packed"] = {"value": round(batch * steps / e2, 2), "ms_per_step": round(e2 / steps * 1e3, 4),
                         "upload_bytes_per_step": int(u8.numel())}
    return pcie


def _parse_cpulist(text):
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


def gpu_numa_cpus(pci_bus_id):
    """CPUs of the NUMA node the GPU with this PCI address ("0000:c1:00.0") hangs off, or None (no sysfs entry, node -1)."""
    try:
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % pci_bus_id.lower()).read())
        if node < 0:
            return None
        return _parse_cpulist(open("/sys/devices/system/node/node%d/cpulist" % node).read()) or None
    except (OSError, ValueError):
        return None


def bind_rank(local_rank, local_world, pci_bus_ids=None):
    """One process per GPU on one node: each rank gets a disjoint slice of the CPUs this job may use (8 conversions start at
    once -- BatchNorm folding in fp64, weight packing -- and 8 x nproc OpenMP threads would fight over the same cores).
    `pci_bus_ids` (one PCI address per local rank, from the HIP device properties): the slice is taken from the CPUs of the
    NUMA node GPU `local_rank` is attached to, shared equally with the other local ranks on that node; without it (dry-host
    runs, no sysfs entry) the job's CPU list is cut into `local_world` contiguous slices.  torch's intra-op pool AND
    OMP_NUM_THREADS are set to the same number (the launcher exports OMP_NUM_THREADS = nproc / gpus; the two must agree).
    Returns the CPU list (unchanged affinity when the job has fewer CPUs than ranks)."""
    import torch
    allowed = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    cpus, mine = allowed, None
    if local_world > 1 and len(allowed) >= local_world:
        if pci_bus_ids and len(pci_bus_ids) == local_world:
            nodes = [gpu_numa_cpus(b) for b in pci_bus_ids]
            if all(n is not None for n in nodes):
                key = tuple(nodes[local_rank])
                peers = [r for r in range(local_world) if tuple(nodes[r]) == key]       # local ranks on the same node
                pool = [c for c in nodes[local_rank] if c in set(allowed)]
                per = len(pool) // len(peers)
                if per >= 1:
                    i = peers.index(local_rank)
                    mine = pool[i * per:(i + 1) * per]
        if mine is None:
            per = len(allowed) // local_world
            mine = allowed[local_rank * per:(local_rank + 1) * per]
        try:
            os.sched_setaffinity(0, mine)
            cpus = mine
        except OSError:
            pass
    threads = max(1, min(len(cpus), 16))
    torch.set_num_threads(threads)
    os.environ["OMP_NUM_THREADS"] = str(threads)
    return cpus


def dry_host(args, world, rank, stdout_guard):
    """Launcher check without a GPU (tests/test_bench_launcher.py): the ORIGINAL-form model on the host, gloo.
    Exercises exactly the spawn / rank binding / barrier / max-over-ranks / n_gpus reporting of the real run;
    its number is not a measurement of the product path and the line says so."""
    import torch
    import torch.distributed as dist
    from pytorchvideo_amd.parallel import gather_logits, shard_range
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    cpus = bind_rank(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    torch.set_num_threads(min(2, len(cpus)))
    if world > 1:
        dist.init_process_group("gloo")
    torch.manual_seed(0)
    model, shape = make_model("x3d_xs_dry")
    model.eval()
    batch = args.batch or 2
    x = synth_input(shape, batch, 1234 + rank)
    how = "torch.distributed (gloo)"
    if os.environ.get("PV_RCCL_LIB"):     # the C communicator with a host-memory librccl double (tests/helpers/rccl_stub.c)
        from pytorchvideo_amd.parallel import HeadComm
        comm = HeadComm()
        recv = torch.empty(batch * world, 400)
        how = "pv_comm over %s" % os.path.basename(comm.library)

        def gather_logits(local, global_batch=None):     # noqa: F811 -- same contract, through pv_comm_all_gather
            return comm.all_gather(local.contiguous(), recv)
    with torch.no_grad():
        for _ in range(args.warmup):
            out = gather_logits(model(x), global_batch=batch * world)
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = gather_logits(model(x), global_batch=batch * world)
        if world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    assert out.shape == (batch * world, 400)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"logits": out})
    # ---- N-GPU readiness beyond the launcher (round-4 verdict, next #7): everything below runs WITHOUT a GPU ----
    ready = {}
    # (1) the rank -> device / CPU binding the real run makes: cuda:LOCAL_RANK, a disjoint CPU slice per rank
    mine = {"rank": rank, "local_rank": local_rank, "device": "cuda:%d" % local_rank, "cpus": cpus}
    bind = [None] * world
    if world > 1:
        dist.all_gather_object(bind, mine)
    else:
        bind = [mine]
    ready["binding"] = bind
    # (2) a ragged global batch (sizes differ by one) through the head collective, against torch.distributed's answer
    if args.dry_ragged:
        gb = batch * world - min(3, world - 1) if world > 1 else batch
        lo, hi = shard_range(gb, rank, world)
        with torch.no_grad():
            local = model(x[: hi - lo]) if hi > lo else torch.zeros(0, 400)
        from pytorchvideo_amd.parallel import gather_logits as torch_gather     # (the local name may be the C communicator's)
        want = torch_gather(local, global_batch=gb)
        if os.environ.get("PV_RCCL_LIB"):
            got = comm.gather_ragged(local, gb)
            ok = bool(torch.equal(got, want))
        else:
            got, ok = want, True
        ready["ragged"] = {"global_batch": gb, "rows": int(got.shape[0]), "sizes": [h - l for l, h in (shard_range(gb, r, world) for r in range(world))],
                           "equal_to_torch_distributed": ok}
        assert got.shape == (gb, 400) and ok
    # (3) the host half of the REAL workload's conversion on every rank at once: BASELINE config of --workload at its per-GPU
    #     batch (x3d_l: 32 clips per GPU, 256 = 8 x 32 over a node), plan statistics must agree across ranks
    if args.dry_convert:
        from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
        wl = WORKLOADS[args.workload]
        m2, shp = make_model(args.workload)
        m2.eval()
        transmute_model(m2, "mi355x")
        shapes = shp if isinstance(shp, list) else [shp]
        xin = [torch.zeros(1, dtype=torch.bfloat16).expand((wl["batch"],) + tuple(sh)) for sh in shapes]
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        st = convert_to_deployable_form(m2, xin if isinstance(shp, list) else xin[0], dtype=torch.bfloat16, emit_only=True)
        st["seconds"] = round(time.perf_counter() - t0, 3)
        allst = [None] * world
        if world > 1:
            dist.all_gather_object(allst, st)
        else:
            allst = [st]
        keys = ("fused", "ops", "arena_bytes", "weight_bytes")
        assert all(tuple(a[k] for k in keys) == tuple(allst[0][k] for k in keys) for a in allst), allst
        ready["convert"] = dict({k: allst[0][k] for k in keys}, concurrent_ranks=world,
                                seconds_max=max(a["seconds"] for a in allst), seconds_min=min(a["seconds"] for a in allst))
        ready["north_star_config"] = {"workload": args.workload + ": " + wl["desc"], "per_gpu_batch": wl["batch"],
                                      "global_batch": wl["batch"] * world}
    if rank == 0:
        stdout_guard.restore()
        print(json.dumps({"metric": "dry-host launcher check (NOT a measurement of the HIP path)",
                          "value": round(batch * world * args.steps / elapsed, 3), "unit": "clips/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "fp32",
                          "data": "synthetic", "config": {"workload": "x3d_xs_dry: original-form model on the host, gloo",
                                                           "per_gpu_batch": batch, "global_batch": batch * world,
                                                           "head_collective": how,
                                                           "local_rank": int(os.environ.get("LOCAL_RANK", "0"))},
                          "readiness": ready}))
    if world > 1:
        dist.destroy_process_group()


class _StdoutToStderr:
    """File descriptor 1 points at stderr while the job runs and comes back for the ONE JSON line: native libraries write
    to the C stdout (RCCL prints a version banner when its first communicator is created; it sits in libc's buffer until exit
    and would land BEHIND the JSON line), and the contract is one JSON line on stdout."""

    def __enter__(self):
        import ctypes
        sys.stdout.flush()
        self._libc = ctypes.CDLL(None)
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def restore(self):
        if self._saved is not None:
            sys.stdout.flush()
            self._libc.fflush(None)          # whatever C code buffered goes to stderr, not behind the JSON line
            os.dup2(self._saved, 1)
            os.close(self._saved)
            self._saved = None

    def __exit__(self, *exc):
        self.restore()
        return False


def main():
    with _StdoutToStderr() as out:
        return _main(out)


def _main(out):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="x3d_m")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: workload's)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--streams", type=int, default=0,
                    help="sub-batches replayed concurrently on their own HIP streams (0: the workload's default)")
    ap.add_argument("--full", action="store_true",
                    help="also the sustained run, the roofline object, the secondary legs and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the logits of the last timed step to DIR/logits.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the MViT-B / SlowFast-R50 / X3D-L legs")
    ap.add_argument("--no-sustained", action="store_true", help="with --full: skip the >= 2 s sustained run")
    ap.add_argument("--no-roofline", action="store_true",
                    help="with --full: skip the per-op profiling passes (rocprofv3 --pmc runs: only the replays are wanted)")
    ap.add_argument("--with-h2d", action="store_true",
                    help="also time steps that upload the (pinned) host input first; reported as pcie_inclusive, never as value")
    ap.add_argument("--head-comm", nargs="?", const="on", default="", choices=["", "on", "require"],
                    help="use the C-driven head collective at N = 1 too (one-rank RCCL communicator); 'require': no fallback")
    ap.add_argument("--dry-host", action="store_true", help="launcher check on the host (gloo, original-form model); no GPU")
    ap.add_argument("--dry-ragged", action="store_true", help="with --dry-host: a ragged global batch through the head collective")
    ap.add_argument("--dry-convert", action="store_true",
                    help="with --dry-host: every rank runs the host half of --workload's conversion at its per-GPU batch, timed")
    ap.add_argument("--tune", default="", help="development knobs k=v,... (pytorchvideo_amd.accelerator.mi355x.tuning / pv_tune_set)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        out.restore()                      # the ranks inherit this process's stdout
        sys.exit(self_spawn(args))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if args.dry_host:
        return dry_host(args, world, rank, out)

    import torch
    import torch.distributed as dist
    if args.tune:
        from pytorchvideo_amd.accelerator.mi355x import tuning
        tuning.apply(args.tune)
    if world > 1:
        lw = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        try:      # PCI addresses of the node's GPUs -> NUMA-local CPU slices (falls back to equal contiguous slices)
            props = [torch.cuda.get_device_properties(i) for i in range(lw)]
            pci = ["%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id) for p in props]
        except Exception:      # noqa: BLE001 -- older torch without the pci_* fields, fewer visible devices than local ranks
            pci = None
        bind_rank(local_rank, lw, pci)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=device)

    setup_head_collective(args, world)
    wl = WORKLOADS[args.workload]
    res, model, x, step, last = run_workload(args.workload, args, world, rank, device, args.steps, args.warmup,
                                             sustained_s=2.0 if args.full and not args.no_sustained else 0.0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"logits": last})
    batch = res["per_gpu_batch"]
    pcie = pcie_leg(model, x, step, batch, args.steps, device) if args.with_h2d else None
    if not args.full or args.no_roofline or rank != 0:
        roof, prof, agg = None, [], {}
    else:
        roof, prof, agg = roofline_of(roofline_session(model, args.workload, batch, device, args), args.workload,
                                      res["value"] / world, res["ms_per_step"])

    # The other BASELINE.json configurations on the same line: MViT-B 32x3 (configs[3], the metric's second model),
    # SlowFast-R50 8x8 (configs[2]) and X3D-L (configs[4]; at N > 1 this is "global batch 32 N sharded over N GPUs").
    # Each leg is a full run_workload: its own warm-up, timed steps with step percentiles, a >= 1 s sustained run and its
    # own roofline object.  `value` of the line stays the X3D-M number at every N so that the driver's scaling curve
    # compares like with like.
    secondary = None
    if args.full and not args.no_secondary and not args.no_roofline and args.workload == "x3d_m" and not args.batch:
        del model, x, step
        torch.cuda.empty_cache()
        secondary = {}
        for w2 in (("mvit_b_32x3", "slowfast_r50", "x3d_l") if world == 1 else ("mvit_b_32x3", "x3d_l")):
            # (the same K timed steps and W warm-up steps as the headline leg: with 10 steps behind 3 warm-up replays one slow
            #  replay -- 20 ms among 5.4 ms ones, X3D-L, profiles/r6/bench_default_line.json -- moved a leg's mean by 20 %)
            r2, m2, x2, _, _ = run_workload(w2, args, world, rank, device, max(10, args.steps), max(3, args.warmup),
                                            sustained_s=0.0 if args.no_sustained else 1.0, prewarm_s=0.3)
            roof2 = None
            if rank == 0 or world == 1:
                roof2, _, _ = roofline_of(roofline_session(m2, w2, r2["per_gpu_batch"], device, args), w2,
                                          r2["value"] / world, r2["ms_per_step"])
            secondary[w2] = {"value": r2["value"], "unit": "clips/s", "ms_per_step": r2["ms_per_step"],
                             "step_ms": r2["step_ms"], "steps": r2["steps"], "warmup": max(3, args.warmup), "prewarm_s": 0.3,
                             "dtype": args.dtype, "n_gpus": world,
                             "sustained": r2.get("sustained"),
                             "config": {"workload": w2 + ": " + WORKLOADS[w2]["desc"], "per_gpu_batch": r2["per_gpu_batch"],
                                        "global_batch": r2["per_gpu_batch"] * world, "streams": r2["streams"]},
                             "roofline": roof2}
            del m2, x2
            roofline_session.keep = None
            torch.cuda.empty_cache()

    if rank == 0:
        line = {
            "metric": "clips/sec forward", "value": res["value"], "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": res["ms_per_step"], "step_ms": res["step_ms"],
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "%s: %s" % (args.workload, wl["desc"]), "per_gpu_batch": batch,
                       "global_batch": batch * world, "parallelism": "dp%d (batch-sharded, logits all_gather)" % world,
                       "head_collective": HEAD["how"],
                       "weights": "random-init conditioned like a checkpoint (pytorchvideo_amd.utils.synthetic_trained_like_weights: BN statistics calibrated on data, block-final gamma U(0.05,0.2)); the instance of tests/test_gpu_full_geometry.py", "hip_graph": not args.no_graph,
                       "streams": res["streams"]},
            "roofline": roof,
        }
        if "sustained" in res:
            line["sustained"] = res["sustained"]
        if secondary is not None:
            line["secondary"] = secondary
        if pcie is not None:
            line["pcie_inclusive"] = pcie
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(args.workload)
        if os.environ.get("PV_BENCH_VERBOSE") == "2":
            for label, kind, ms, alg_bytes, flops in prof:
                print("  op %-60s %8.4f ms %8.1f GB/s %8.2f TF/s" % (label, ms, alg_bytes / max(ms, 1e-9) / 1e6,
                                                                   flops / max(ms, 1e-9) / 1e9), file=sys.stderr)
        if os.environ.get("PV_BENCH_VERBOSE"):
            for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                print("  %-16s n=%3d %8.3f ms  %8.1f GB/s  %7.2f TF/s" % (
                    k, v[0], v[1], v[2] / max(v[1], 1e-9) / 1e6, v[3] / max(v[1], 1e-9) / 1e9), file=sys.stderr)
        out.restore()
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)        # anything native code still prints at teardown (communicator destruction) goes to stderr
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
