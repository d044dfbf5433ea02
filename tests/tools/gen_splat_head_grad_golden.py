"""Generates tests/golden/splat_head_grad.npz by running the REFERENCE's own predictor under autograd (tests/tools/ref_import.py, CPU
torch, build container only -- the reference does not travel; the fixture is data only).

GaussianSplatPredictor_gtunet.forward on the inputs of tests/golden/splat_head.npz with the U-Net replaced by a fixed map, as
gen_golden.py does, but with ``net_out`` and ``depth`` requiring grad: seeded cotangents on the seven outputs, squre_clip 10000 and 0.3.
Stored: the cotangents (cot_<key>) and the reference's gradients d_net_out / d_depth (and d_net_out_clip / d_depth_clip), float32.
"""
import copy
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KEYS = ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest", "unet_depth")
npy = lambda t: t.detach().cpu().numpy().astype(np.float32)


def main():
    ref_import.install()
    cfg = yaml.safe_load(open(os.path.join(ref_import.REF, "config/imagenetgs_256x256_v1.yaml")))
    g = np.load(os.path.join(OUT, "splat_head.npz"))
    with ref_import.Cuda2Cpu():
        import src.gaussian_predictor as gp
        cfg32 = copy.deepcopy(cfg)
        cfg32['model']['training_resolution'] = 32
        torch.manual_seed(0)
        pred = gp.GaussianSplatPredictor_gtunet(cfg32).eval()
        assert np.array_equal(pred.ray_dirs.numpy(), g["ray_dirs"])
        net_out = torch.from_numpy(g["net_out"]).requires_grad_()
        depth = torch.from_numpy(g["depth"]).requires_grad_()
        v2w, quat = torch.from_numpy(g["v2w"]), torch.from_numpy(g["quat"])
        B, res = net_out.shape[0], net_out.shape[-1]

        class _Fixed(torch.nn.Module):       # replaces the U-Net by a fixed 23-channel map
            def forward(self, x, **kw):
                return net_out
        pred.network_with_offset = _Fixed()
        x_dummy = torch.zeros(B, 1, 4, res, res)
        gen = torch.Generator().manual_seed(11)
        cots, saved = None, {}
        for tag, clip in (("", 10000.0), ("_clip", 0.3)):
            out = pred(x_dummy, v2w.unsqueeze(1), quat.unsqueeze(1), unet_depth=depth, squre_clip=clip)
            if cots is None:
                for k in KEYS:
                    assert np.array_equal(npy(out[k]), g["out_" + k]), k          # the very forward of splat_head.npz
                cots = {k: torch.randn(out[k].shape, generator=gen) for k in KEYS}
            d_net, d_depth = torch.autograd.grad([out[k] for k in KEYS], [net_out, depth], [cots[k] for k in KEYS])
            saved["d_net_out" + tag], saved["d_depth" + tag] = npy(d_net), npy(d_depth)
    path = os.path.join(OUT, "splat_head_grad.npz")
    np.savez_compressed(path, **{"cot_" + k: npy(v) for k, v in cots.items()}, **saved)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
