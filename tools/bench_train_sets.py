"""Times one training-shaped rasterizer step -- B = 8 sets of 65,536 pixel-ordered Gaussians x 4 views at 256 x 256, forward with
auxiliary planes + backward -- by three routes (run on the GPU box) and prints ONE JSON line:

  (a) batched   one f3dg_forward_sets (SAVE_AUX | SETS_AUX) + one f3dg_backward_sets for all 32 views
                (rasterize_views(save_aux=True, n_sets=8) + rasterize_backward_raw(n_sets=8))
  (b) per_image a loop over the 8 images of 4-view calls (rasterize_views(save_aux=True) + rasterize_backward_raw: one set per call)
  (c) one_view  32 calls of GaussianRasterizer_GOF (the drop-in autograd Function), each followed by its backward

Same Gaussians, cameras and cotangents in all three; the cotangent is on the raster, so no route runs an epilogue. What is timed is a
whole step (32 views forward and backward) between two HIP events on the current stream, after WARM untimed steps of that route; the
routes are timed in alternating rounds (a, b, c, a, b, c, ...) so that drift of the shared host hits all of them alike, and the JSON
holds the median, minimum and maximum of the per-round means. (a) and (b) check the instance count once per forward
(one blocking status read per call), as (c)'s drop-in call does.

The GPU work runs in a child process under a time limit; a failing child ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, B, V, WARM, STEPS, ROUNDS = 256, 8, 4, 3, 10, 5


def child(res, n_sets, n_views, warm, steps, rounds):
    import torch
    sys.path.insert(0, ROOT)
    import f3dgaus_amd as f3d
    from f3dgaus_amd import _lib, synthetic
    from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw
    dev = torch.device("cuda:0")
    P = res * res
    sets = [synthetic.make_pixel_gaussians(res, s0=0.01, seed=17 * b, device=dev) for b in range(n_sets)]
    for g in sets:
        g["shs"] = torch.cat([g["features_dc"], g["features_rest"]], 1).contiguous()
    cat = {k: torch.cat([g[k] for g in sets], 0).contiguous() for k in ("xyz", "opacity", "scaling", "rotation", "shs")}
    cams = synthetic.orbit_cameras(max(n_views, 8), resolution=res, device=dev)
    vm, pm, cp = (cams[k][:n_views].contiguous() for k in ("viewmatrix", "projmatrix", "campos"))
    vm_all, pm_all, cp_all = (t.repeat(n_sets, *([1] * (t.ndim - 1))).contiguous() for t in (vm, pm, cp))       # set-major: b * V + v
    bg = torch.zeros(3, device=dev)
    tan = cams["tanfovx"]
    dpix = torch.randn(n_sets * n_views, 9, res, res, generator=torch.Generator().manual_seed(11)).to(dev)
    kw = dict(image_height=res, image_width=res, tanfovx=tan, tanfovy=tan, sh_degree=1, save_aux=True)
    state = {}

    def route_a():
        out, radii, ws = f3d.rasterize_views(cat["xyz"], cat["opacity"], vm_all, pm_all, cp_all, bg, sh=cat["shs"], scales=cat["scaling"],
                                             rotations=cat["rotation"], n_sets=n_sets, workspace=state.get("a"), **kw)
        state["a"] = ws
        return rasterize_backward_raw(ws, cat["xyz"], cat["shs"], None, cat["scaling"], cat["rotation"], radii, dpix, 1, vm_all, pm_all,
                                      cp_all, bg, tan, tan, 0.0, 1.0, n_sets=n_sets)

    def route_b():
        for b, g in enumerate(sets):
            out, radii, ws = f3d.rasterize_views(g["xyz"], g["opacity"], vm, pm, cp, bg, sh=g["shs"], scales=g["scaling"],
                                                 rotations=g["rotation"], workspace=state.get("b"), **kw)
            state["b"] = ws
            rasterize_backward_raw(ws, g["xyz"], g["shs"], None, g["scaling"], g["rotation"], radii, dpix[b * n_views:(b + 1) * n_views], 1,
                                   vm, pm, cp, bg, tan, tan, 0.0, 1.0)

    leaves = [{k: g[k].clone().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs")} for g in sets]
    settings = [f3d.GaussianRasterizationSettings_GOF(res, res, tan, tan, 0.0, torch.zeros(0), bg, 1.0, vm[v], pm[v], 1, cp[v], False, False)
                for v in range(n_views)]
    rasterizers = [f3d.GaussianRasterizer_GOF(s) for s in settings]

    def route_c():
        for b, lf in enumerate(leaves):
            for v in range(n_views):
                m2d = torch.zeros_like(lf["xyz"], requires_grad=True)
                color, _ = rasterizers[v](means3D=lf["xyz"], means2D=m2d, shs=lf["shs"], opacities=lf["opacity"], scales=lf["scaling"],
                                          rotations=lf["rotation"])
                color.backward(dpix[b * n_views + v])
        for lf in leaves:
            for t in lf.values():
                t.grad = None

    routes = {"batched": route_a, "per_image": route_b, "one_view": route_c}
    L = _lib.lib()
    launches = {}
    for name, fn in routes.items():
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        L.f3dg_debug_launch_count(1)
        fn()
        torch.cuda.synchronize()
        launches[name] = int(L.f3dg_debug_launch_count(1))
    per_round = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_round[name].append(e0.elapsed_time(e1) / steps)
    # the three routes compute the same gradients: the batched sums against the per-image ones, once, outside the timed windows
    ga = route_a()
    gb = []
    for b, g in enumerate(sets):
        _, radii, ws = f3d.rasterize_views(g["xyz"], g["opacity"], vm, pm, cp, bg, sh=g["shs"], scales=g["scaling"], rotations=g["rotation"], **kw)
        gb.append(rasterize_backward_raw(ws, g["xyz"], g["shs"], None, g["scaling"], g["rotation"], radii, dpix[b * n_views:(b + 1) * n_views], 1,
                                         vm, pm, cp, bg, tan, tan, 0.0, 1.0))
    agree = {}
    for k in ("dL_dopacity", "dL_dsh", "dL_dmeans3D"):
        ref = torch.cat([g[k] for g in gb], 0)
        agree[k] = float((ga[k] - ref).abs().max() / ref.abs().max())
    res_ = {name: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v),
                   "library_launches_per_step": launches[name]} for name, v in per_round.items()}
    res_["batched_vs_per_image_max_rel_diff"] = agree
    print("RESULT " + json.dumps(res_), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--res", type=int, default=RES)
    ap.add_argument("--sets", type=int, default=B)
    ap.add_argument("--views", type=int, default=V)
    ap.add_argument("--warmup", type=int, default=WARM)
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--timeout", type=float, default=420.0)
    a = ap.parse_args()
    if a.child:
        return child(a.res, a.sets, a.views, a.warmup, a.steps, a.rounds)
    result = {"bench": "train_sets", "resolution": a.res, "sets": a.sets, "views_per_set": a.views, "gaussians_per_set": a.res * a.res,
              "warmup_steps": a.warmup, "timed_steps_per_round": a.steps, "rounds": a.rounds}
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for k in ("res", "sets", "views", "warmup", "steps", "rounds")
                                                                      for x in ("--" + k, str(getattr(a, k)))]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(json.dumps({**result, "error": "time limit"}))
        return 1
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        print(json.dumps({**result, "error": f"exit status {p.returncode}"}))
        return 1
    result["routes"] = json.loads(line[-1][7:])
    r = result["routes"]
    result["batched_over_per_image"] = r["batched"]["ms_per_step_median"] / r["per_image"]["ms_per_step_median"]
    result["batched_over_one_view"] = r["batched"]["ms_per_step_median"] / r["one_view"]["ms_per_step_median"]
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
