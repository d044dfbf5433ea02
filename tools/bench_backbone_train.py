"""Times one backbone forward + backward under autograd at B = 8 images, 256 x 256 (run on the GPU box): the torch route
(``cfg['model']['backbone_autograd'] = 'torch'``: torch's GroupNorm / SiLU / bias / add operators between MIOpen's convolutions) against
the fused route (``'fused'``: ``f3dg_group_norm_silu_forward_stats`` / ``f3dg_group_norm_silu_backward_dtype`` / ``f3dg_residual_join_forward`` /
``_backward_dtype``) in both layouts; prints ONE JSON line and, with ``--markdown PATH``, writes the table of profiles/backbone_train.md.

``--dtype fp32`` (default) is float32 throughout. ``--dtype bf16 | fp16``: the fused route with ``cfg['model']['backbone_train_dtype']``
set to it (16-bit activations through the kernels forward and backward), and as its yardstick the torch route under the same
``torch.autocast``; the kernels alone then run on 16-bit tensors (half the bytes per element).

step      ``GaussianSplatPredictor_gtunet(..., head=False)`` on 8 images + ``backward`` of a fixed cotangent on ``net_out``, parameters'
          gradients included; the three variants share their weights. Peak memory: ``torch.cuda.max_memory_allocated`` over one step of
          the variant, minus what was allocated before it (weights, inputs): the step's own activations, gradients and scratch.
kernels   the GroupNorm + SiLU backward alone on the backbone's largest call, [8, 128, 256, 256] with a pre_bias: the NCHW kernel (one
          workgroup per (sample, group) slab, which re-reads its 2 x 1 MiB of x and grad_y after reducing them), the channels-last three
          (partials, finish, apply), and torch's own backward of group_norm + silu on the same tensors. Bytes per element if the second
          read is served by a cache: 8 read + 4 written = 12; if it goes to HBM again: 20 (16-bit: 6 and 10).

Method: HIP events around ``TIMED`` calls after ``WARM`` warm-ups of that same call (the first of which also pays MIOpen's find step); the
variants alternate within one process, ``ROUNDS`` times; the figure is the median round with the smallest and the largest beside it. The
measurement is a child process under its own time limit, whose progress lines are passed on."""
import argparse
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, B, WARM, TIMED, ROUNDS, PEAK = 256, 8, 2, 5, 5, 8.0e12
K_SHAPE, K_TIMED = (8, 128, 256, 256), 20
TAIL = "## Figures from other runs"
VARIANTS = (("torch", "torch", "nchw"), ("fused_nchw", "fused", "nchw"), ("fused_nhwc", "fused", "nhwc"))


def _timed(torch, fn, timed):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(timed):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / timed * 1e-3


def _alternate(torch, variants, timed):
    """{name: median / min / max seconds per call over the rounds}, the variants taking turns."""
    times = {name: [] for name in variants}
    for r in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(_timed(torch, fn, timed))
        print(f"round {r + 1} / {ROUNDS} done", flush=True)
    return {name: {"median_s": sorted(t)[len(t) // 2], "min_s": min(t), "max_s": max(t)} for name, t in times.items()}


DTYPES = ("fp32", "bf16", "fp16")


def _kernel_calls(torch, dev, dtype="fp32"):
    """{name: call} of the GroupNorm + SiLU backward alone at K_SHAPE: this build's two layouts and torch's own; and what they keep alive."""
    td, code = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype], DTYPES.index(dtype)
    from f3dgaus_amd import _lib
    from f3dgaus_amd.diff_gof_rasterization import _stream
    N, Cc, H, W = K_SHAPE
    G, HW = 32, H * W
    x = (torch.randn(K_SHAPE, device=dev) * 1.5 + 0.7).to(td)
    gy = torch.randn(K_SHAPE, device=dev).to(td)
    w, b, pb = torch.rand(Cc, device=dev) + 0.5, torch.rand(Cc, device=dev) - 0.5, torch.randn(Cc, device=dev) * 0.3
    L, p = _lib.lib(), _lib.ptr
    calls = {}
    keep = []
    for nhwc in (0, 1):
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        xl, gl = x.contiguous(memory_format=fmt), gy.contiguous(memory_format=fmt)
        y, dx = torch.empty_like(xl), torch.empty_like(xl)
        stats = torch.empty(N, G, 2, device=dev)
        mom = torch.empty(L.f3dg_group_norm_nhwc_scratch_bytes(N, HW, G) // 8 + 1, dtype=torch.float64, device=dev)
        _lib.check(L.f3dg_group_norm_silu_forward_stats(_stream(), code, nhwc, N, Cc, HW, G, p(xl), p(pb), p(w), p(b), 1e-6, 1, p(y), p(stats), p(mom),
                                                        mom.numel() * 8), "f3dg_group_norm_silu_forward_stats")
        scratch = torch.empty(L.f3dg_group_norm_silu_backward_scratch_bytes(N, Cc, HW, G, nhwc) // 8 + 1, dtype=torch.float64, device=dev)
        dw, db, dpb = (torch.empty(Cc, device=dev) for _ in range(3))
        args = (code, N, Cc, HW, G, nhwc, p(xl), p(pb), p(w), p(b), p(stats), 1, p(gl), p(dx), p(dw), p(db), p(dpb), p(scratch), scratch.numel() * 8)
        keep.append((xl, gl, y, dx, stats, mom, scratch, dw, db, dpb))
        calls["kernel_nhwc" if nhwc else "kernel_nchw"] = lambda args=args: _lib.check(L.f3dg_group_norm_silu_backward_dtype(_stream(), *args), "f3dg_group_norm_silu_backward_dtype")
    xt, wt, bt, pbt = (t.clone().requires_grad_() for t in (x, w, b, pb))
    yt = torch.nn.functional.silu(torch.nn.functional.group_norm(xt + pbt.to(td).reshape(1, -1, 1, 1), G, wt.to(td), bt.to(td), 1e-6))
    calls["torch_bwd"] = lambda: torch.autograd.grad(yt, (xt, wt, bt, pbt), gy, retain_graph=True)
    return calls, keep


def kernel_only(name, dtype="fp32"):
    """Three calls of one variant and nothing else: the process to put under a counter pass (``rocprofv3 --pmc FETCH_SIZE -- python
    tools/bench_backbone_train.py --kernel-only kernel_nchw``: the bytes the L2 fetched say whether the NCHW kernel's re-read hit it)."""
    import torch
    sys.path.insert(0, ROOT)
    calls, keep = _kernel_calls(torch, torch.device("cuda:0"), dtype)
    for _ in range(3):
        calls[name]()
    torch.cuda.synchronize()
    return 0


def child(dtype="fp32"):
    import torch
    sys.path.insert(0, ROOT)
    from f3dgaus_amd import cameras
    from f3dgaus_amd import gaussian_predictor as gp
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {}

    # ---- the kernels alone
    calls, keep = _kernel_calls(torch, dev, dtype)
    res["kernels"] = _alternate(torch, calls, K_TIMED)
    res["kernels"]["elements"] = K_SHAPE[0] * K_SHAPE[1] * K_SHAPE[2] * K_SHAPE[3]
    del calls, keep
    torch.cuda.empty_cache()
    print("kernels done", flush=True)

    # ---- the whole backbone step
    preds = {}
    state = None
    for name, route, layout in VARIANTS:
        cfg = cameras.default_cfg(RES)
        cfg["model"]["backbone_autograd"], cfg["model"]["backbone_layout"] = route, layout
        if route == "fused":
            cfg["model"]["backbone_train_dtype"] = dtype
        pred = gp.GaussianSplatPredictor_gtunet(cfg)
        if state is None:
            state = pred.state_dict()
        pred.load_state_dict(state)
        preds[name] = pred.to(dev).eval()
    xin = torch.rand(B, 1, 4, RES, RES, device=dev)
    depth = torch.rand(B, 1, RES, RES, device=dev) * 2 + 6.667
    v2w = torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(B, 1, 1, 1)
    quat = torch.tensor([1.0, 0, 0, 0], device=dev).reshape(1, 1, 4).repeat(B, 1, 1)
    cot = torch.randn(B, 23, RES, RES, device=dev)

    half = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(dtype)

    def step(pred):
        pred.zero_grad(set_to_none=True)
        # (the torch route has no 16-bit option of its own: its yardstick is the same backbone under the same autocast)
        with torch.autocast("cuda", dtype=half, enabled=half is not None and pred.backbone_autograd == "torch"):
            net_out, _ = pred(xin, v2w, quat, unet_depth=depth, head=False)
        net_out.float().backward(cot)

    steps = {name: (lambda pred=pred: step(pred)) for name, pred in preds.items()}
    for name, fn in steps.items():          # first use: MIOpen's find step for this variant's convolution problems
        fn()
        torch.cuda.synchronize()
        print(f"first step of {name} done", flush=True)
    res["step"] = _alternate(torch, steps, TIMED)
    for name, fn in steps.items():
        preds[name].zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res["step"][name]["peak_bytes"] = torch.cuda.max_memory_allocated() - base
        preds[name].zero_grad(set_to_none=True)
    print("RESULT " + json.dumps(res), flush=True)


def _ms(c):
    return "%.2f ms (%.2f .. %.2f)" % (c["median_s"] * 1e3, c["min_s"] * 1e3, c["max_s"] * 1e3)


def markdown(r):
    s, k = r["step"], r["kernels"]
    n = k["elements"]
    t0 = s["torch"]
    dtype = r.get("dtype", "fp32")
    wide = dtype == "fp32"
    lo, hi = (12, 20) if wide else (6, 10)
    name = {"fp32": "float32", "bf16": "bfloat16", "fp16": "float16"}[dtype]
    torch_label = "`backbone_autograd = 'torch'` (NCHW)" + ("" if wide else " under `torch.autocast(%s)`" % name)
    fused = "`'fused'`" if wide else "`'fused'`, `backbone_train_dtype = '%s'`" % dtype
    rate = lambda c, bpe: "%.2f TB/s" % (n * bpe / c["median_s"] * 1e-12)
    rows = [
        "# Training through the fused backbone: one forward + backward step",
        "",
        "`python tools/bench_backbone_train.py%s --markdown profiles/backbone_train.md` on an MI355X: B = %d images, %d x %d, %s, one view per"
        % ("" if wide else " --dtype " + dtype, B, RES, RES, name),
        "image. HIP events around %d steps (kernels alone: %d calls) after %d warm-ups; the variants alternate within one process, %d rounds;"
        % (TIMED, K_TIMED, WARM, ROUNDS),
        "median round (smallest .. largest). The yardstick is the torch route of the same run; no bar hangs on the ratio.",
        "",
        "| backbone forward + backward, 8 images | time per step | against torch | peak memory of the step | against torch |",
        "|---|---|---|---|---|",
    ]
    for key, label in (("torch", torch_label), ("fused_nchw", fused + ", NCHW"), ("fused_nhwc", fused + ", `backbone_layout = 'nhwc'`")):
        c = s[key]
        rows.append("| %s | %s | %.2f x | %.2f GiB | %.2f x |" % (label, _ms(c), c["median_s"] / t0["median_s"], c["peak_bytes"] / 2.0 ** 30,
                                                               c["peak_bytes"] / t0["peak_bytes"]))
    rows += [
        "",
        "Peak memory: `torch.cuda.max_memory_allocated` over one step minus what was allocated before it (weights, inputs).",
        "",
        "| GroupNorm + SiLU backward alone, [8, 128, 256, 256] %s with pre_bias (%.0f M elements) | time per call | if the re-read is cached (%d B / element) | if it is not (%d B / element) |"
        % (name, n * 1e-6, lo, hi),
        "|---|---|---|---|",
        "| `f3dg_group_norm_silu_backward_dtype`, NCHW: one workgroup per (sample, group), 2 x %s MiB re-read | %s | %s | %s |"
        % ("1" if wide else "0.5", _ms(k["kernel_nchw"]), rate(k["kernel_nchw"], lo), rate(k["kernel_nchw"], hi)),
        "| `f3dg_group_norm_silu_backward_dtype`, channels-last: partials, finish, apply | %s | %s | %s |"
        % (_ms(k["kernel_nhwc"]), rate(k["kernel_nhwc"], lo), rate(k["kernel_nhwc"], hi)),
        "| torch autograd of `silu(group_norm(x + pre_bias))`, backward alone | %s | | |" % _ms(k["torch_bwd"]),
        "",
        "The two right-hand columns are the same time read two ways: the bytes the call moves if the second read of `x` and `grad_y` is served",
        "by a cache (%d B read + %d B written per element) or goes to memory again (%d B). A rate in the last column above what the device can" % (lo * 2 // 3, lo // 3, hi),
        "stream (%.0f TB/s peak) would mean the re-read is cached; a rate in the middle column far below it says nothing either way." % (PEAK * 1e-12),
        ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--markdown", help="write the table of profiles/backbone_train.md to this path")
    ap.add_argument("--dtype", choices=DTYPES, default="fp32", help="activations of the fused route (backbone_train_dtype); 16-bit: the torch route runs "
                    "under the same autocast and the kernels alone on 16-bit tensors")
    ap.add_argument("--step-timeout", type=float, default=900.0)
    ap.add_argument("--kernel-only", choices=("kernel_nchw", "kernel_nhwc", "torch_bwd"), help="three calls of that variant alone, for a counter pass")
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(a.kernel_only, a.dtype)
    if a.child:
        return child(a.dtype)
    result = {"bench": "backbone_train", "dtype": a.dtype, "B": B, "resolution": RES, "warmup": WARM, "timed": TIMED, "kernel_timed": K_TIMED, "rounds": ROUNDS}
    # the child's progress lines are passed on as they come (stderr); its RESULT line is kept
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--dtype", a.dtype], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    timer = threading.Timer(a.step_timeout, p.kill)
    timer.start()
    line = []
    for l in p.stdout:
        if l.startswith("RESULT "):
            line.append(l)
        else:
            sys.stderr.write(l)
            sys.stderr.flush()
    p.wait()
    expired = not timer.is_alive()
    timer.cancel()
    if p.returncode != 0 or not line:
        print(json.dumps({**result, "error": "time limit" if expired else f"exit status {p.returncode}"}))
        return 1
    result.update(json.loads(line[-1][7:]))
    if a.markdown:
        # what a page holds from other runs (counter passes, the suite's accuracy figures) stands below TAIL and is kept
        tail = ""
        if os.path.exists(a.markdown):
            old = open(a.markdown).read()
            if TAIL in old:
                tail = old[old.index(TAIL):]
        with open(a.markdown, "w") as f:
            f.write(markdown(result) + tail)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
