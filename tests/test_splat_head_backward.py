"""CPU pins of the splat head's backward: the torch restatement that serves as gradient truth (tests/splat_head_truth.py) against the
reference's fixtures -- forward and gradients --, and the host-side argument checks of f3dg_splat_head_backward (no GPU call)."""
import ctypes as C

import numpy as np
import pytest
import torch

import splat_head_truth as T
from oracle import splat_head as sh_oracle


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_restatement_forward_is_the_reference_forward():
    """float32 forward of the restatement == splat_head.npz / splat_head_clip.npz (the reference's outputs) and oracle/splat_head.py,
    to the 3e-6 the splat head's own tests use."""
    inp, g = T.load_inputs()
    with torch.no_grad():
        out = T.splat_head_torch(**inp)
        outc = T.splat_head_torch(**inp, squre_clip=0.3)
    want = sh_oracle.splat_head(*(inp[k].numpy() for k in ("net_out", "depth", "ray_dirs", "v2w", "quat")))
    for k in T.KEYS:
        assert out[k].dtype == torch.float32 and out[k].shape == g["out_" + k].shape, k
        assert _rel(out[k].numpy(), g["out_" + k]) < 3e-6, k
        assert _rel(out[k].numpy(), want[k]) < 3e-6, k
    gc = np.load(T.os.path.join(T.GOLD, "splat_head_clip.npz"))
    assert _rel(outc["xyz"].numpy(), gc["out_xyz"]) < 3e-6
    wantc = sh_oracle.splat_head(*(inp[k].numpy() for k in ("net_out", "depth", "ray_dirs", "v2w", "quat")), squre_clip=0.3)
    assert _rel(outc["xyz"].numpy(), wantc["xyz"]) < 3e-6
    # float64 runs too, and agrees
    with torch.no_grad():
        out64 = T.splat_head_torch(inp["net_out"].double(), inp["depth"].double(), inp["ray_dirs"], inp["v2w"], inp["quat"])
    assert all(out64[k].dtype == torch.float64 and _rel(out64[k].numpy(), g["out_" + k]) < 3e-6 for k in T.KEYS)


@pytest.mark.parametrize("tag,clip", [("", 10000.0), ("_clip", 0.3)])
def test_restatement_float32_gradients_reproduce_the_reference_autograd(tag, clip):
    """g32 of the restatement against the gradients the reference's own predictor returned (tests/tools/gen_splat_head_grad_golden.py).
    Both are float32 evaluations of the same ops, each within E_ref of the float64 truth, so they differ by at most 2 * E_ref * max|g64|
    per channel group (they are bit-identical where the host's torch kernels are)."""
    inp, _ = T.load_inputs()
    cots, g = T.load_cotangents()
    g32 = T.restatement_grads(inp, cots, clip, torch.float32)
    g64 = T.restatement_grads(inp, cots, clip, torch.float64)
    ref = (torch.from_numpy(g["d_net_out" + tag]), torch.from_numpy(g["d_depth" + tag]))
    assert ref[0].shape == g32[0].shape == (2, 23, 32, 32) and ref[1].shape == g32[1].shape == (2, 1, 32, 32)
    bounds = T.group_bounds(g32, g64)
    for name, t in T.by_group(*ref).items():
        e_ref, m = bounds[name]
        d = float((t - T.by_group(*g32)[name]).abs().max())
        print(f"{name:8s} E_ref {e_ref:.3e}  |g32 - reference| / max {d / m:.3e}")
        assert m > 0 and d <= 2 * e_ref * m, (name, d, e_ref, m)
        # and the truth itself is the reference's, to float32
        assert float((t.double() - T.by_group(*g64)[name]).abs().max()) <= 2 * e_ref * m, name
    if clip < 10:       # the clamp is active somewhere and removes gradient there
        plain = np.load(T.os.path.join(T.GOLD, "splat_head_grad.npz"))["d_net_out"]
        assert np.abs(plain[:, :3] - g["d_net_out_clip"][:, :3]).max() > 0
        assert np.array_equal(plain[:, 3:], g["d_net_out_clip"][:, 3:])


def test_splat_head_backward_host_side_errors(f3d):
    """F3DG_ERR_BAD_ARG before any HIP call: NULL required pointers, non-positive sizes, a window that does not fit n_total."""
    from f3dgaus_amd import _lib
    L = _lib.lib()
    null = None
    buf = (C.c_char * 1024)()
    one = C.cast(buf, C.c_void_p)
    call = lambda B, H, W, req, n_total, n_offset, d_net: L.f3dg_splat_head_backward(
        null, B, H, W, *req, 1.0, n_total, n_offset, *([null] * 7), d_net, null)
    assert call(2, 32, 32, [null] * 5, 1024, 0, null) == _lib.ERR_BAD_ARG
    assert call(2, 32, 32, [one] * 5, 1024, 0, null) == _lib.ERR_BAD_ARG               # d_net_out is required
    for i in range(5):                                                               # each of the five inputs is required
        req = [one] * 5
        req[i] = null
        assert call(2, 32, 32, req, 1024, 0, one) == _lib.ERR_BAD_ARG, i
    assert call(0, 32, 32, [one] * 5, 1024, 0, one) == _lib.ERR_BAD_ARG
    assert call(2, 0, 32, [one] * 5, 1024, 0, one) == _lib.ERR_BAD_ARG
    assert call(2, 32, -1, [one] * 5, 1024, 0, one) == _lib.ERR_BAD_ARG
    assert call(2, 32, 32, [one] * 5, 1023, 0, one) == _lib.ERR_BAD_ARG                # n_total < H*W
    assert call(2, 32, 32, [one] * 5, 2048, 1025, one) == _lib.ERR_BAD_ARG             # n_total < n_offset + H*W
    assert call(2, 32, 32, [one] * 5, 2048, -1, one) == _lib.ERR_BAD_ARG


def test_splat_head_python_refusals_need_no_gpu(f3d):
    """No CPU fallback under autograd either: host tensors are refused before anything else."""
    x = torch.zeros(1, 23, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        f3d.splat_head(x, torch.zeros(1, 1, 4, 4), torch.zeros(1, 3, 4, 4), torch.eye(4)[None], torch.zeros(1, 4))
