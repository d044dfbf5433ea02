"""Times the two pieces that training through the cycle aggregation adds, at B = 8 images, V = 8 novel views, 256 x 256 (run on the GPU
box), against the torch composition each replaces; prints ONE JSON line and, with ``--markdown PATH``, writes the table of
profiles/cycle_train.md.

hand-off   ``f3dg_cycle_inputs_backward`` alone (the kernel on prepared cotangents), and ``cycle_inputs`` forward + backward under
           autograd, against torch: cat([r[:, :, :3].clamp(0, 1), r[:, :, 7:8]], 2).transpose(0, 1) and r[:, :, 6:7].transpose(0, 1) under
           autograd -- backward alone (graph retained) and forward + backward. Bytes the kernel has to move per (frame, pixel):
           3 raster planes + 4 + 1 cotangent planes read, 9 planes written = 68 B.
merge      ``splat_head_merge`` of the K = 1 + V passes, forward + backward, against K autograd ``splat_head`` calls + ``torch.cat`` per
           key, forward + backward, on the same inputs and the same merged cotangents. Bytes per Gaussian: forward 96 B read + 96 B
           written, backward 96 B inputs + 96 B cotangents read + 96 B written = 480 B.

Method: HIP events around ``TIMED`` calls (a tenth as many of the merge) after ``WARM`` warm-ups of that same call; the variants of a section alternate within one
process, ``ROUNDS`` times, and the figure is the median round with the smallest and the largest beside it. Each section is a child
process under its own time limit; the first failing one ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, B, V, WARM, TIMED, ROUNDS, PEAK = 256, 8, 8, 10, 1000, 5, 8.0e12


def _timed(torch, fn, timed=TIMED):
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


def _alternate(torch, variants, timed=TIMED):
    """{name: [seconds per call, one per round]}, the variants taking turns."""
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(_timed(torch, fn, timed))
    return {name: {"median_s": sorted(t)[len(t) // 2], "min_s": min(t), "max_s": max(t)} for name, t in times.items()}


def child(what):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import f3dgaus_amd as f3d
    from f3dgaus_amd import _lib, cameras
    from f3dgaus_amd.diff_gof_rasterization import _stream
    from f3dgaus_amd.gaussian_predictor import GAUSSIAN_KEYS, _KEY_SHAPE
    from f3dgaus_amd.gaussian_renderer import cycle_inputs
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    HW = RES * RES
    if what == "handoff":
        raster = (torch.randn(B * V, 9, RES, RES, device=dev) * 0.6 + 0.5).requires_grad_()
        gx, gz = torch.randn(V, B, 4, RES, RES, device=dev), torch.randn(V, B, 1, RES, RES, device=dev)
        d_raster = torch.empty_like(raster)
        L, p = _lib.lib(), _lib.ptr
        args = (B, V, RES, RES, p(raster), p(gx), p(gz), p(d_raster))

        def torch_fwd(r):
            r5 = r.reshape(B, V, 9, RES, RES)
            return torch.cat([r5[:, :, :3].clamp(0, 1), r5[:, :, 7:8]], 2).transpose(0, 1), r5[:, :, 6:7].transpose(0, 1)

        kept = torch_fwd(raster)
        # the results the timed variants produce are the same (tests/test_cycle_autograd_gpu.py holds them bit for bit at a small shape)
        ours, = torch.autograd.grad(cycle_inputs(raster, B, V), raster, [gx, gz])
        theirs, = torch.autograd.grad(torch_fwd(raster), raster, [gx, gz])
        assert torch.equal(ours, theirs)
        res = _alternate(torch, {
            "kernel": lambda: _lib.check(L.f3dg_cycle_inputs_backward(_stream(), *args), "f3dg_cycle_inputs_backward"),
            "torch_bwd": lambda: torch.autograd.grad(kept, raster, [gx, gz], retain_graph=True),
            "ours_fwd_bwd": lambda: torch.autograd.grad(cycle_inputs(raster, B, V), raster, [gx, gz]),
            "torch_fwd_bwd": lambda: torch.autograd.grad(torch_fwd(raster), raster, [gx, gz]),
        })
        res["bytes"] = B * V * HW * 68
    else:
        K = 1 + V
        cfg = cameras.default_cfg(RES)
        rig = cameras.OrbitRig(cfg)
        ob = rig.orbit(V)
        nets, depths = [], []
        for _ in range(K):
            net = torch.randn(B, 23, RES, RES, device=dev) * 0.5
            net[:, 4:7] = net[:, 4:7] * 0.3 + float(np.log(0.01))
            nets.append(net.requires_grad_())
            depths.append((torch.rand(B, 1, RES, RES, device=dev) * 2 + 6.667).requires_grad_())
        v2ws = [rig.canonical.view_to_world_transforms[0, 0]] + [ob.view_to_world_transforms[v, 0] for v in range(V)]
        quats = [rig.canonical.source_cv2wT_quat[0, 0]] + [ob.source_cv2wT_quat[v, 0] for v in range(V)]
        v2ws = [m.reshape(1, 4, 4).repeat(B, 1, 1).to(dev) for m in v2ws]
        quats = [q.reshape(1, 4).repeat(B, 1).to(dev) for q in quats]
        px = torch.linspace(-RES // 2 + 0.5, RES // 2 - 0.5, RES) / f3d.gaussian_predictor.fov2focal(cfg["model"]["fov"] * np.pi / 180, RES)
        gx, gy = torch.meshgrid(px, px, indexing="xy")
        ray_dirs = torch.stack([gx, gy, torch.ones_like(gx)]).unsqueeze(0).to(dev)
        cots = [torch.randn((B, K * HW) + _KEY_SHAPE[k], device=dev) for k in GAUSSIAN_KEYS]
        leaves = nets + depths

        def ours():
            pc = f3d.splat_head_merge(nets, depths, ray_dirs, v2ws, quats)
            return torch.autograd.grad([pc[k] for k in GAUSSIAN_KEYS], leaves, cots)

        def theirs():
            sets = [f3d.splat_head(nets[k], depths[k], ray_dirs, v2ws[k], quats[k]) for k in range(K)]
            return torch.autograd.grad([torch.cat([s[k] for s in sets], 1) for k in GAUSSIAN_KEYS], leaves, cots)

        assert all(torch.equal(a, b) for a, b in zip(ours(), theirs()))
        res = _alternate(torch, {"ours_fwd_bwd": ours, "torch_fwd_bwd": theirs}, timed=TIMED // 10)
        res["bytes"] = B * K * HW * 480
    print("RESULT " + json.dumps(res), flush=True)


def _ms(c):
    return "%.3f ms (%.3f .. %.3f)" % (c["median_s"] * 1e3, c["min_s"] * 1e3, c["max_s"] * 1e3)


def markdown(r):
    h, m = r["handoff"], r["merge"]
    rate = lambda nbytes, c: "%.2f TB/s, %.0f %% of 8 TB/s" % (nbytes / c["median_s"] * 1e-12, 100 * nbytes / c["median_s"] / PEAK)
    return "\n".join([
        "# Training through the cycle aggregation: hand-off adjoint and merged head",
        "",
        "`python tools/bench_cycle_train.py --markdown profiles/cycle_train.md` on an MI355X: B = %d images, V = %d novel views, %d x %d." % (B, V, RES, RES),
        "HIP events around %d calls (merge: %d) after %d warm-ups of the same call; the variants of a section alternate within one process, %d"
        % (TIMED, TIMED // 10, WARM, ROUNDS),
        "rounds; median round (smallest .. largest). Every timed pair was first checked `torch.equal` on these inputs.",
        "",
        "| hand-off adjoint (%.1f MB to move) | time per call | |" % (h["bytes"] * 1e-6),
        "|---|---|---|",
        "| `f3dg_cycle_inputs_backward`, the kernel alone | %s | %s |" % (_ms(h["kernel"]), rate(h["bytes"], h["kernel"])),
        "| torch autograd of clamp / slices / cat / transpose, backward alone | %s | %.1f x the kernel |"
        % (_ms(h["torch_bwd"]), h["torch_bwd"]["median_s"] / h["kernel"]["median_s"]),
        "| `cycle_inputs` under autograd, forward + backward | %s | |" % _ms(h["ours_fwd_bwd"]),
        "| the torch composition, forward + backward | %s | %.1f x |"
        % (_ms(h["torch_fwd_bwd"]), h["torch_fwd_bwd"]["median_s"] / h["ours_fwd_bwd"]["median_s"]),
        "",
        "| merged head, K = %d passes, forward + backward (%.1f MB to move) | time per call | |" % (1 + V, m["bytes"] * 1e-6),
        "|---|---|---|",
        "| `splat_head_merge`: one node, cotangents read in place | %s | %s |" % (_ms(m["ours_fwd_bwd"]), rate(m["bytes"], m["ours_fwd_bwd"])),
        "| K autograd `splat_head` + `torch.cat` per key | %s | %.1f x |"
        % (_ms(m["torch_fwd_bwd"]), m["torch_fwd_bwd"]["median_s"] / m["ours_fwd_bwd"]["median_s"]),
        "",
        "The rates are the bytes the algorithm has to move over the call's time, host launches included (the merge is 2 x K launches and the",
        "allocation of its outputs): end-to-end figures of the call, not a kernel's share of peak. No bar hangs on them; the comparison is the",
        "torch composition, which is what a caller had before.",
        ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("handoff", "merge"))
    ap.add_argument("--markdown", help="write the table of profiles/cycle_train.md to this path")
    ap.add_argument("--step-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    result = {"bench": "cycle_train", "B": B, "V": V, "resolution": RES, "warmup": WARM, "timed": TIMED, "rounds": ROUNDS, "peak_bytes_per_s": PEAK}
    for what in ("handoff", "merge"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({**result, "error": f"{what}: time limit"}))
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            print(json.dumps({**result, "error": f"{what}: exit status {p.returncode}"}))
            return 1
        result[what] = json.loads(line[-1][7:])
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(markdown(result))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
