"""Time the backbone's GroupNorm+SiLU kernels of two builds of the library against each other (profiles/backbone_kernels.md).

    python tools/bench_backbone_kernels.py --parent /path/to/parent/libf3dg_hip.so [--calls 100] [--repeats 3] [--out FILE.md]

Both libraries are loaded into one process and called through the C ABI on the same tensors: channels-last and NCHW GroupNorm+SiLU with
the folded bias at (16, 128, 256, 256) and (16, 512, 32, 32), float32 and bfloat16. A measurement is the median over `--calls` calls, each
between two device events, after a warm-up, both builds writing the same output buffer; it is repeated `--repeats` times per library, the two libraries alternating. The table
gives the median of the repeats and the parent's spread (max - min of its repeats); the outputs of the two builds are compared too."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from f3dgaus_amd import _lib                                    # noqa: E402

SHAPES = ((16, 128, 256, 256), (16, 512, 32, 32))


def load(path):
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if "group_norm" in name:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--this", default=_lib.LIB_PATH)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    libs = (("parent", load(a.parent)), ("this", load(a.this)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    lines = ["| layout | shape | type | parent ms | this ms | this - parent | parent's spread | max abs difference of the outputs |",
             "|---|---|---|---:|---:|---:|---:|---:|"]
    for shape in SHAPES:
        N, Cc, H, W = shape
        HW, groups = H * W, 32
        torch.manual_seed(0)
        w, b, pb = torch.rand(Cc, device=dev) + 0.5, torch.rand(Cc, device=dev) - 0.5, torch.randn(Cc, device=dev) * 0.3
        for dt, kd in ((torch.float32, 0), (torch.bfloat16, 1)):            # F3DG_F32, F3DG_BF16
            x = (torch.randn(N * Cc * HW, device=dev) * 2 + 0.5).to(dt)
            for layout in ("nhwc", "nchw"):
                outs, times, scratch = {}, {k: [] for k, _ in libs}, {}

                def call(L, y):
                    mom, nbytes = None, 0
                    if layout == "nhwc":
                        mom = scratch.get(id(L))                     # (each build sizes its own scratch)
                        if mom is None:
                            mom = scratch[id(L)] = torch.empty(L.f3dg_group_norm_nhwc_scratch_bytes(N, HW, groups) // 8 + 1, dtype=torch.float64, device=dev)
                        nbytes = mom.numel() * 8
                    rc = L.f3dg_group_norm_silu_forward(stream, kd, 1 if layout == "nhwc" else 0, N, Cc, HW, groups, p(x), p(pb), p(w), p(b), 1e-6, 1, p(y),
                                                        None, p(mom) if mom is not None else None, nbytes)
                    assert rc == 0, rc

                def measure(L, y):
                    for _ in range(5):
                        call(L, y)
                    torch.cuda.synchronize()
                    ms = []
                    for _ in range(a.calls):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); call(L, y); e1.record()
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    return statistics.median(ms)

                y = torch.empty_like(x)                  # ONE output buffer for both builds: where a buffer lies moves these times by a few per cent
                for _ in range(a.repeats):
                    for name, L in libs:
                        times[name].append(measure(L, y))
                        outs[name] = y.clone()
                diff = float((outs["this"].float() - outs["parent"].float()).abs().max())
                tp, tt = statistics.median(times["parent"]), statistics.median(times["this"])
                spread = max(times["parent"]) - min(times["parent"])
                lines.append(f"| {layout} | {N} x {Cc} x {H} x {W} | {'fp32' if dt == torch.float32 else 'bf16'} | {tp:.4f} | {tt:.4f} | {tt - tp:+.4f} | "
                             f"{spread:.4f} | {diff:.2e} |")
                print(lines[-1], " repeats parent", ["%.4f" % t for t in times["parent"]], "this", ["%.4f" % t for t in times["this"]], flush=True)
            del x
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
