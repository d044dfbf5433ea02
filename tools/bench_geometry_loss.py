"""Times forward + backward of the five geometry terms (depth-normal consistency with the alpha weight, distortion, masked depth, masked
normal, alpha) through the fused route -- losses.geometry_loss: f3dg_geometry_loss_forward / _backward -- against the route the package
offered before: f3dg_render_epilogue_view for the two derived maps, the terms as torch operations on the maps with their autograd graph,
and f3dg_render_epilogue_backward for the maps' cotangents. 32 frames of 256 x 256, starting from a raster LEAF, so no rasterizer time is
counted. Prints ONE JSON line. Device events around runs that end in a synchronise; both routes alternate in one process; the median of
the rounds is reported. ``--count-launches`` adds the kernel launches of one forward + backward of each route (the library's own launch
counter, and every device kernel as the torch profiler sees them).

    python tools/bench_geometry_loss.py [--rounds 15] [--frames 32] [--res 256] [--count-launches]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import f3dgaus_amd  # noqa: E402,F401
from f3dgaus_amd import _lib, losses, synthetic  # noqa: E402
from f3dgaus_amd.diff_gof_rasterization import _stream  # noqa: E402

WEIGHTS = dict(w_depth_normal=0.05, w_distortion=0.1, w_depth=0.5, w_normal=0.2, w_alpha=1.0)


class EpilogueMaps(torch.autograd.Function):
    """(normal_world, depth_normal) of a raster [F, 9, H, W] by f3dg_render_epilogue_view, f3dg_render_epilogue_backward behind it: what
    render_views(differentiable=True) runs for its two derived maps."""

    @staticmethod
    def forward(ctx, raster, wv, fx, fy):
        F, _, H, W = raster.shape
        nw, dn = (torch.empty((F, 3, H, W), dtype=torch.float32, device=raster.device) for _ in range(2))
        _lib.check(_lib.lib().f3dg_render_epilogue_view(_stream(), F, H, W, _lib.ptr(raster), _lib.ptr(wv), fx, fy, _lib.ptr(nw), _lib.ptr(dn)),
                   "f3dg_render_epilogue_view")
        ctx.save_for_backward(raster, wv)
        ctx.f = (fx, fy)
        return nw, dn

    @staticmethod
    def backward(ctx, g_nw, g_dn):
        raster, wv = ctx.saved_tensors
        F, _, H, W = raster.shape
        d = torch.zeros_like(raster)
        _lib.check(_lib.lib().f3dg_render_epilogue_backward(_stream(), F, H, W, _lib.ptr(raster), _lib.ptr(wv), *ctx.f, _lib.ptr(g_nw.contiguous()),
                                                            _lib.ptr(g_dn.contiguous()), _lib.ptr(d)), "f3dg_render_epilogue_backward")
        return d, None, None, None


def torch_route(raster, wv, fx, fy, depth_t, normal_t, alpha_t, mask):
    """The same loss from the maps, in torch operations."""
    nw, dn = EpilogueMaps.apply(raster, wv, fx, fy)
    alpha = raster[:, 7]
    t0 = (alpha.detach() * (1 - (nw * dn).sum(1))).mean()
    t1 = raster[:, 8].mean()
    t2 = (mask * (raster[:, 6] - depth_t).abs()).mean()
    t3 = (mask * (1 - (torch.nn.functional.normalize(raster[:, 3:6], dim=1) * normal_t).sum(1))).mean()
    t4 = (alpha - alpha_t).abs().mean()
    w = WEIGHTS
    return w["w_depth_normal"] * t0 + w["w_distortion"] * t1 + w["w_depth"] * t2 + w["w_normal"] * t3 + w["w_alpha"] * t4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def count_launches(fn):
    """(launches of libf3dg_hip.so, device kernels the torch profiler saw or None) of one call."""
    L = _lib.lib()
    torch.cuda.synchronize()
    L.f3dg_debug_launch_count(1)
    fn()
    torch.cuda.synchronize()
    own = int(L.f3dg_debug_launch_count(1))
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                      and "memset" not in e.name.lower())
    except Exception as exc:        # a count is a diagnostic: the times above do not depend on it
        print("profiler unavailable:", exc, file=sys.stderr)
        kernels = None
    return own, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry_loss needs a HIP device: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    F, R = args.frames, args.res
    g = torch.Generator(device=dev).manual_seed(0)
    u = lambda *s: torch.rand(s, generator=g, device=dev)
    n = lambda *s: torch.randn(s, generator=g, device=dev)
    x = torch.arange(R, device=dev).float()
    raster = n(F, 9, R, R)
    raster[:, 6] = 2.0 + 0.3 * torch.sin(0.05 * x).reshape(1, 1, R) * torch.cos(0.04 * x).reshape(1, R, 1) + 0.01 * n(F, R, R)
    raster[:, 3:6] = 0.5 * n(F, 3, R, R) + torch.tensor([0., 0., 1.], device=dev).reshape(1, 3, 1, 1)
    raster[:, 7] = u(F, R, R)
    raster.requires_grad_()
    cam = synthetic.orbit_cameras(F, R, device=dev)
    wv, cfg = cam["viewmatrix"].reshape(F, 16).contiguous(), cam["cfg"]
    FoV = cfg["model"]["fov"] * math.pi / 180
    fx = fy = float(R / (2 * math.tan(FoV / 2.)))
    depth_t = raster[:, 6].detach() + 0.1 * n(F, R, R)
    normal_t = torch.nn.functional.normalize(n(F, 3, R, R), dim=1)
    alpha_t, mask = (u(F, R, R) < 0.5).float(), (u(F, R, R) < 0.7).float()

    def fused():
        raster.grad = None
        loss = losses.geometry_loss(raster, wv, cfg, alpha_weight=True, depth_target=depth_t, normal_target=normal_t, alpha_target=alpha_t,
                                    mask=mask, **WEIGHTS)
        loss.backward()
        return loss.detach(), raster.grad

    def eager():
        raster.grad = None
        loss = torch_route(raster, wv, fx, fy, depth_t, normal_t, alpha_t, mask)
        loss.backward()
        return loss.detach(), raster.grad

    (lf, gf), (le, ge) = fused(), eager()
    scale = float(ge.abs().max())
    agree = {"loss_fused": float(lf), "loss_torch": float(le), "grad_max_abs_diff_over_max": float((gf - ge).abs().max()) / scale}
    tf, te = [], []
    for _ in range(2):
        timed(fused), timed(eager)
    for _ in range(args.rounds):
        tf.append(timed(fused)[0])
        te.append(timed(eager)[0])
    f_ms, e_ms = statistics.median(tf), statistics.median(te)
    out = {"tool": "bench_geometry_loss", "device": torch.cuda.get_device_name(0), "frames": F, "res": R, "rounds": args.rounds,
           "fused_ms": round(f_ms, 4), "fused_min_ms": round(min(tf), 4), "torch_ms": round(e_ms, 4), "torch_min_ms": round(min(te), 4),
           "torch_over_fused": round(e_ms / f_ms, 2), "fused_faster": f_ms < e_ms, "agreement": agree,
           "note": "forward + backward of all five terms from a raster leaf; torch route = f3dg_render_epilogue_view + torch ops + autograd + "
                   "f3dg_render_epilogue_backward"}
    if args.count_launches:
        (of, kf), (oe, ke) = count_launches(fused), count_launches(eager)
        out["launches"] = {"fused_library": of, "fused_all_kernels": kf, "torch_library": oe, "torch_all_kernels": ke}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
