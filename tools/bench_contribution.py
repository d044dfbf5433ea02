"""Times the per-Gaussian contribution pass and what pruning by it buys, on the real image's merged set (tests/real_data.py: 589,824
pixel-aligned Gaussians) over a 128-view orbit at 256^2, 32 views per call.

  (a) the contribution pass (f3dg_contribution) per call and in total, beside the exact compositing stage of the forwards it follows;
  (b) the comparator a user had before: a save_aux forward + rasterize_backward_raw with a unit gradient on one colour channel, whose
      dL_dcolors is the sum of the blend weights per view -- both routes alternate in one process after a warm-up each, device events,
      medians of the rounds; and the largest relative difference between sum_weight and that gradient (a cross-check, not a gate);
  (c) the shares of the set with touched == 0, max_weight < 0.01 and < 0.05;
  (d) orbit views/s, exact and fast arithmetic, on the full set and on each pruned set, with the RGB PSNR of the pruned frames against the
      full set's.
Prints ONE JSON line.

    python tools/bench_contribution.py [--rounds 5] [--views 128] [--image 256] [--views-per-call 32]
"""
import argparse
import copy
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f3dgaus_amd as f3d  # noqa: E402
from f3dgaus_amd import _lib, synthetic  # noqa: E402
from f3dgaus_amd.diff_gof_rasterization.backward import rasterize_backward_raw  # noqa: E402


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--views-per-call", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contribution needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    from real_data import real_merged_set
    g = real_merged_set(dev)
    P, res, step = g["xyz"].shape[0], args.image, args.views_per_call
    pc = {k: t[None].contiguous() for k, t in g.items()}
    cams = synthetic.orbit_cameras(args.views, resolution=res, device=dev)
    cfg = cams["cfg"]
    wv, fp, cc = cams["viewmatrix"], cams["projmatrix"], cams["campos"]
    V = wv.shape[0]
    tanfov = math.tan(cfg['model']['fov'] * math.pi / 360)
    bg = torch.zeros(3, device=dev)
    shs = torch.cat([g["features_dc"], g["features_rest"]], 1).contiguous()
    kw = dict(image_height=res, image_width=res, tanfovx=tanfov, tanfovy=tanfov, sh=shs, scales=g["scaling"], rotations=g["rotation"],
              sh_degree=cfg['model']['max_sh_degree'])
    chunks = [(v0, min(step, V - v0)) for v0 in range(0, V, step)]
    unit = torch.zeros(step, 9, res, res, device=dev)
    unit[:, 0] = 1.0

    def forward(v0, n, ws, **more):
        return f3d.rasterize_views(g["xyz"], g["opacity"], wv[v0:v0 + n], fp[v0:v0 + n], cc[v0:v0 + n], bg, workspace=ws, **kw, **more)

    def route_pass(stats, ws):
        """exact inference forwards + the contribution pass: (ms of the passes per call, workspace)"""
        ms = []
        for v0, n in chunks:
            _, _, ws = forward(v0, n, ws, exact=True)
            a, b = events()
            a.record()
            f3d.contribution_raw(ws, P, res, res, n, tanfov, tanfov, stats=stats)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms, ws

    def route_backward(ws, keep=None):
        """save_aux forwards + the backward with a unit gradient on the red channel: (ms of the backwards per call, workspace)"""
        ms = []
        for v0, n in chunks:
            _, radii, ws = forward(v0, n, ws, save_aux=True)
            a, b = events()
            a.record()
            grads = rasterize_backward_raw(ws, g["xyz"], shs, None, g["scaling"], g["rotation"], radii, unit[:n], cfg['model']['max_sh_degree'],
                                           wv[v0:v0 + n], fp[v0:v0 + n], cc[v0:v0 + n], bg, tanfov, tanfov, 0.0, 1.0)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
            if keep is not None:
                keep += grads["dL_dcolors"][:, :, 0].double().sum(0)
            del grads
        return ms, ws

    # warm-up of both routes; the statistics and the comparator's sums come from it
    stats = f3d.GaussianContribution(P, dev)
    _, ws_a = route_pass(stats, None)
    grad_sum = torch.zeros(P, dtype=torch.float64, device=dev)
    _, ws_b = route_backward(None, grad_sum)
    again = f3d.GaussianContribution(P, dev)
    route_pass(again, ws_a)
    repeatable = bool(torch.equal(again.raw, stats.raw))

    t_pass, t_bwd, t_comp, t_comp_aux = [], [], [], []
    st, nc = (C.c_double * 5)(), C.c_int(0)
    for _ in range(args.rounds):
        L.f3dg_profile_enable(1)
        ms, ws_a = route_pass(f3d.GaussianContribution(P, dev), ws_a)
        _lib.check(L.f3dg_profile_collect(st, C.byref(nc)), "f3dg_profile_collect")
        t_pass.append(ms)
        t_comp.append(st[2])
        ms, ws_b = route_backward(ws_b)
        _lib.check(L.f3dg_profile_collect(st, C.byref(nc)), "f3dg_profile_collect")
        L.f3dg_profile_enable(0)
        t_bwd.append(ms)
        t_comp_aux.append((st[2], st[3], st[4]))
    med = statistics.median
    pass_total, bwd_total = med(sum(r) for r in t_pass), med(sum(r) for r in t_bwd)
    sw = stats.sum_weight
    seen = sw >= 1e-3
    rel = ((sw - grad_sum).abs() / sw.clamp_min(1e-30))[seen]
    num_rendered = ws_a.num_rendered

    # (c) what the statistics say about the set
    tc, mw = stats.touched, stats.max_weight
    shares = {"touched_0": float((tc == 0).double().mean()), "max_weight_below_0.01": float((mw < 0.01).double().mean()),
              "max_weight_below_0.05": float((mw < 0.05).double().mean()), "stop_only": float(((stats.blended == 0) & (stats.stops > 0)).double().mean())}

    # (d) the orbit on the full set and on the pruned sets
    sets = {"full": pc, "touched>=1": f3d.prune_gaussians(pc, 0, stats)[0], "max_weight>=0.01": f3d.prune_gaussians(pc, 0, stats, min_max_weight=0.01)[0],
            "max_weight>=0.05": f3d.prune_gaussians(pc, 0, stats, min_max_weight=0.05)[0]}

    def orbit(gs, exact, keep_frames):
        c = copy.deepcopy(cfg)
        c['model']['raster_exact'] = bool(exact)
        frames, ws = [], None
        a, b = events()
        a.record()
        for v0, n in chunks:
            out = f3d.render_views(gs, 0, wv[v0:v0 + n], fp[v0:v0 + n], cc[v0:v0 + n], bg, c, workspace=ws, epilogue=False, channels="rgb_depth_alpha")
            ws = out["workspace"]
            if keep_frames:
                frames.append(out["raster"][:, :3].clone())
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (torch.cat(frames) if keep_frames else None)

    def psnr(a, b):
        mse = float(((a.double() - b.double()) ** 2).mean())
        return None if mse == 0 else round(10.0 * math.log10(1.0 / mse), 2)

    full_frames = {e: orbit(pc, e, True)[1] for e in (True, False)}
    orbit_rows = {}
    for name, gs in sets.items():
        row = {"gaussians": int(gs["xyz"].shape[1])}
        for e in (True, False):
            label = "exact" if e else "fast"
            _, fr = orbit(gs, e, True)                                  # warm-up; the frames for the comparison
            row[label + "_bit_identical"] = bool(torch.equal(fr.view(torch.int32), full_frames[e].view(torch.int32)))
            row[label + "_rgb_psnr_db"] = psnr(fr, full_frames[e])      # None: identical
            del fr
            ts = [orbit(gs, e, False)[0] for _ in range(args.rounds)]
            row[label + "_ms"] = round(med(ts), 3)
            row[label + "_views_per_s"] = round(V / (med(ts) * 1e-3), 1)
        orbit_rows[name] = row

    r3 = lambda x: round(x, 3)
    print(json.dumps({
        "tool": "bench_contribution", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "gaussians": P, "views": V, "image": res,
        "views_per_call": step, "instances_last_call": num_rendered, "statistics_bitwise_repeatable": repeatable,
        "contribution_pass_ms_per_call": [r3(med(r[i] for r in t_pass)) for i in range(len(chunks))], "contribution_pass_ms_total": r3(pass_total),
        "exact_compositing_ms_total_same_calls": r3(med(t_comp)),
        "comparator_backward_ms_per_call": [r3(med(r[i] for r in t_bwd)) for i in range(len(chunks))], "comparator_backward_ms_total": r3(bwd_total),
        "comparator_stages_ms_total": {"save_aux_compositing_forward": r3(med(x[0] for x in t_comp_aux)), "compositing_backward": r3(med(x[1] for x in t_comp_aux)),
                                       "per_gaussian_backward": r3(med(x[2] for x in t_comp_aux))},
        "backward_over_pass": round(bwd_total / pass_total, 2), "pass_cheaper": bool(pass_total < bwd_total),
        "cross_check": {"gaussians_with_sum_weight_above_1e-3": int(seen.sum()), "max_relative_difference": float(rel.max()) if rel.numel() else 0.0,
                        "max_absolute_difference": float((sw - grad_sum).abs().max())},
        "shares": {k: round(v, 5) for k, v in shares.items()}, "orbit": orbit_rows,
        "note": "pass / backward ms: device events around f3dg_contribution / rasterize_backward_raw alone, medians of the rounds, routes alternating in one "
                "process; the forwards they follow are timed by the library's stage events; orbit: device events around the 128 views, 32 per call, "
                "rgb_depth_alpha channels, no epilogue"}))


if __name__ == "__main__":
    main()
