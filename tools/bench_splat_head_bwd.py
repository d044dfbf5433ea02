"""Times f3dg_splat_head_backward at B = 8 and B = 64 images of 256 x 256 (run on the GPU box) and prints ONE JSON line.

Per batch size: the kernel's time (HIP events around 50 launches after 10 warm-ups), its fraction of the 8 TB/s HBM roofline on the bytes
it has to move, and the time of the only alternative without the kernel: float32 torch autograd of the restatement of the reference's
lines (tests/splat_head_truth.py) on the same device and inputs -- its backward alone (graph retained) and forward + backward.

Bytes counted per call: B * HW * 288 + HW * 12
    read    net_out 23 x 4 + depth 4                        = 96 B per Gaussian
    read    upstream gradients (3 + 1 + 3 + 4 + 3 + 9 + 1) x 4 = 96 B per Gaussian
    written d_net_out 23 x 4 + d_depth 4                    = 96 B per Gaussian
    read    ray_dirs 3 x 4 per PIXEL, once (shared by the B images; the 16 + 4 camera floats per image are not counted)

Every GPU step is a child process under its own time limit; the first failing step ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, WARM, TIMED, PEAK = 256, 10, 50, 8.0e12


def child(what, B):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import f3dgaus_amd as f3d
    from f3dgaus_amd import _lib, cameras
    from f3dgaus_amd.diff_gof_rasterization import _stream
    import splat_head_truth as T
    dev = torch.device("cuda:0")
    HW = RES * RES
    torch.manual_seed(0)
    cfg = cameras.default_cfg(RES)
    ob = cameras.OrbitRig(cfg).orbit(8)
    net = torch.randn(B, 23, RES, RES, device=dev) * 0.5
    net[:, 4:7] = net[:, 4:7] * 0.3 - 4.6
    depth = torch.rand(B, 1, RES, RES, device=dev) * 2 + 6.667
    v2w = ob.view_to_world_transforms[:, 0][torch.arange(B) % 8].to(dev).contiguous()
    quat = ob.source_cv2wT_quat[:, 0][torch.arange(B) % 8].to(dev).contiguous()
    from oracle import splat_head as sh_oracle
    ray_dirs = torch.from_numpy(sh_oracle.init_ray_dirs(RES, cfg["model"]["fov"])).to(dev)
    cots = [torch.randn((B, HW) + f3d.gaussian_predictor._KEY_SHAPE[k], device=dev) for k in T.KEYS]

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(TIMED):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / TIMED * 1e-3

    res = {}
    if what == "kernel":
        d_net, d_dep = torch.empty_like(net), torch.empty_like(depth)
        L = _lib.lib()
        p = _lib.ptr
        args = (B, RES, RES, p(net), p(depth), p(ray_dirs), p(v2w.reshape(B, 16)), p(quat), 10000.0, HW, 0, *[p(c) for c in cots], p(d_net), p(d_dep))
        res["kernel_s"] = timed(lambda: _lib.check(L.f3dg_splat_head_backward(_stream(), *args), "f3dg_splat_head_backward"))
        out = f3d.gaussian_predictor.allocate_gaussians(B, HW, dev)
        res["forward_kernel_s"] = timed(lambda: f3d.splat_head(net, depth, ray_dirs, v2w, quat, out=out))
    else:
        net.requires_grad_()
        depth.requires_grad_()
        fwd = lambda: T.splat_head_torch(net, depth, ray_dirs, v2w, quat)
        out = fwd()
        outs = [out[k] for k in T.KEYS]
        res["torch_bwd_s"] = timed(lambda: torch.autograd.grad(outs, [net, depth], cots, retain_graph=True))
        del out, outs

        def both():
            o = fwd()
            torch.autograd.grad([o[k] for k in T.KEYS], [net, depth], cots)
        res["torch_fwd_bwd_s"] = timed(both)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("kernel", "torch"))
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--step-timeout", type=float, default=120.0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.B)
    result = {"bench": "splat_head_backward", "resolution": RES, "warmup": WARM, "timed": TIMED, "peak_bytes_per_s": PEAK, "cases": []}
    for B in (8, 64):
        nbytes = B * RES * RES * 288 + RES * RES * 12
        case = {"B": B, "gaussians": B * RES * RES, "bytes": nbytes}
        for what in ("kernel", "torch"):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--B", str(B)], capture_output=True, text=True,
                                   timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({**result, "error": f"{what} B={B}: time limit"}))
                return 1
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                print(json.dumps({**result, "error": f"{what} B={B}: exit status {p.returncode}"}))
                return 1
            case.update(json.loads(line[-1][7:]))
        case["kernel_bytes_per_s"] = nbytes / case["kernel_s"]
        case["roofline_fraction"] = case["kernel_bytes_per_s"] / PEAK
        case["speedup_vs_torch_bwd"] = case["torch_bwd_s"] / case["kernel_s"]
        case["faster_than_torch"] = case["kernel_s"] < case["torch_bwd_s"]
        result["cases"].append(case)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
