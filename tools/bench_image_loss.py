"""Times the fused image loss (f3dgaus_amd.losses.photometric_loss, forward + backward) on the GPU box against the same loss written with
torch.nn.functional.conv2d -- the formulation of the reference's utils/loss_utils.py that a user would otherwise run -- and prints ONE
JSON line.

Shapes: [8, 4, 3, 256, 256] (the training shape of profiles/render_sets_backward.md) and [16, 8, 3, 256, 256]. Per shape, after 10
warm-up calls, HIP events around 50 calls of
    fused_fwd_bwd_s     photometric_loss(render, target).backward()   (render requires grad)
    fwd_kernel_s        f3dg_ssim_forward alone, training configuration: no map, the three derivative planes, the per-plane sums
    bwd_kernel_s        f3dg_ssim_backward alone, per-plane weights (no gradient plane)
    torch_fwd_bwd_s     (1 - 0.2) * l1 + 0.2 * (1 - ssim) with five grouped conv2d calls, forward + backward
The two kernel times are set against the bytes DESIGN.md section 3e-bis says they move (halo re-reads are served by L2 and not counted):
    forward   8 B read (a, b) + 12 B written (three planes)            = 20 B per pixel of every plane
    backward  12 B read (three planes) + 8 B read (a, b) + 4 B written = 24 B per pixel
Every GPU step is a child process under its own time limit; the fused steps of both shapes run first, the torch steps (whose first
conv2d call of a shape may spend a long time in MIOpen's search) last, and the first failing step ends the run: what was measured up
to there is printed, the rest is reported as not measured.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8, 4, 3, 256, 256), (16, 8, 3, 256, 256))
WARM, TIMED, PEAK, LAMBDA = 10, 50, 8.0e12, 0.2
FWD_BYTES_PER_PIXEL, BWD_BYTES_PER_PIXEL = 20, 24


def _timed(torch, fn):
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


def _torch_loss(torch, window):
    F = torch.nn.functional

    def ssim(a, b):
        C = a.shape[1]
        conv = lambda x: F.conv2d(x, window, padding=5, groups=C)
        mu1, mu2 = conv(a), conv(b)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()
    return lambda a, b: (1.0 - LAMBDA) * torch.abs(a - b).mean() + LAMBDA * (1.0 - ssim(a, b))


def child(what, shape):
    import math
    import torch
    sys.path.insert(0, ROOT)
    import f3dgaus_amd  # noqa: F401
    from f3dgaus_amd import _lib, losses
    from f3dgaus_amd.diff_gof_rasterization import _stream
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    render = torch.rand(shape, generator=gen).to(dev).requires_grad_()
    target = (render.detach().cpu() + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1).to(dev)
    res = {}
    if what == "fused":
        def both():
            render.grad = None
            losses.photometric_loss(render, target, LAMBDA).backward()
        res["fused_fwd_bwd_s"] = _timed(torch, both)
        res["loss"] = float(losses.photometric_loss(render, target, LAMBDA))
        L, p = _lib.lib(), _lib.ptr
        H, W = shape[-2:]
        n = render.numel() // (H * W)
        a, b = render.detach().reshape(n, H, W), target.reshape(n, H, W)
        planes = [torch.empty_like(a) for _ in range(3)]
        nbytes = L.f3dg_ssim_partials_bytes(n, W, H)
        partials, sums = torch.empty(nbytes // 4, device=dev), torch.empty(n, 3, device=dev)
        res["fwd_kernel_s"] = _timed(torch, lambda: _lib.check(L.f3dg_ssim_forward(
            _stream(), n, W, H, p(a), p(b), None, *[p(t) for t in planes], p(partials), nbytes, p(sums)), "f3dg_ssim_forward"))
        w = torch.zeros(n, 3, device=dev)
        w[:, 0], w[:, 1] = -LAMBDA / a.numel(), (1.0 - LAMBDA) / a.numel()
        grad = torch.empty_like(a)
        res["bwd_kernel_s"] = _timed(torch, lambda: _lib.check(L.f3dg_ssim_backward(
            _stream(), n, W, H, p(a), p(b), None, p(w), *[p(t) for t in planes], p(grad)), "f3dg_ssim_backward"))
    else:
        g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)])
        g = (g / g.sum()).unsqueeze(1)
        window = g.mm(g.t()).float().expand(3, 1, 11, 11).contiguous().to(dev)
        loss = _torch_loss(torch, window)
        a, b = render.detach().reshape(-1, *shape[-3:]).requires_grad_(), target.reshape(-1, *shape[-3:])

        def both():
            a.grad = None
            loss(a, b).backward()
        res["torch_fwd_bwd_s"] = _timed(torch, both)
        res["torch_loss"] = float(loss(a, b))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("fused", "torch"))
    ap.add_argument("--shape", type=int, nargs=5, default=list(SHAPES[0]))
    ap.add_argument("--step-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, tuple(a.shape))
    result = {"bench": "image_loss", "warmup": WARM, "timed": TIMED, "peak_bytes_per_s": PEAK, "lambda_dssim": LAMBDA, "cases": []}
    cases = {shape: {"shape": list(shape)} for shape in SHAPES}
    status = 0
    for what, shape in [("fused", s) for s in SHAPES] + [("torch", s) for s in SHAPES]:
        label = f"{what} {'x'.join(map(str, shape))}"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--shape", *map(str, shape)],
                               capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            result["error"] = f"{label}: time limit of {a.step_timeout:.0f} s; later steps not measured"
            status = 1
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            result["error"] = f"{label}: exit status {p.returncode}; later steps not measured"
            status = 1
            break
        cases[shape].update(json.loads(line[-1][7:]))
    for shape in SHAPES:
        c = cases[shape]
        pixels = 1
        for d in shape:
            pixels *= d
        c["pixels"] = pixels
        for k, per in (("fwd", FWD_BYTES_PER_PIXEL), ("bwd", BWD_BYTES_PER_PIXEL)):
            if k + "_kernel_s" in c:
                c[k + "_bytes"] = per * pixels
                c[k + "_bytes_per_s"] = per * pixels / c[k + "_kernel_s"]
                c[k + "_roofline_fraction"] = c[k + "_bytes_per_s"] / PEAK
        if "fused_fwd_bwd_s" in c and "torch_fwd_bwd_s" in c:
            c["torch_over_fused"] = c["torch_fwd_bwd_s"] / c["fused_fwd_bwd_s"]
        result["cases"].append(c)
    print(json.dumps(result))
    return status


if __name__ == "__main__":
    sys.exit(main())
