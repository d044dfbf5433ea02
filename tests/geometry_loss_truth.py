"""Truth for the fused geometry losses (f3dg_geometry_loss_forward / _backward, f3dgaus_amd.losses.geometry_sums): a dtype-generic torch
restatement of the five terms on top of ``epilogue_truth.epilogue_torch`` (the reference's post-processing of a rendered frame), its
autograd in float32 and float64 on the CPU, the fixtures and the tolerance rules the GPU tests share.

Per pixel, with N, D = ``epilogue_torch``'s normal_world and depth_normal, n^ = F.normalize(raster[3:6]), m the mask:
    term 0  w (1 - <N, D>)            w = 1, or raster[7] DETACHED with ``alpha_weight``
    term 1  raster[8]
    term 2  m |raster[6] - depth_target|
    term 3  m (1 - <n^, normal_target>)
    term 4  |raster[7] - alpha_target|
A term whose target is None is identically zero.

Tolerance rules.
  Sums, per frame and term (N = H W pixels, t32 / t64 the restatement's per-pixel terms in float32 / float64):
      |s_kernel - s64| <= 4 sum_p |t32(p) - t64(p)|  +  N 2^-24 sum_p |t64(p)|
  the restatement's own float32 error summed without cancellation, with the project's margin of 4, plus the
  worst-case bound of any float32 summation order. With N <= 1024, one dropped or doubled pixel of average size exceeds it 16-fold.
  Gradients: ``epilogue_truth.check_groups`` (kernel <= 4 E_ref against float64) on channels 3..5 and 6; the other channels are exact."""
import torch

import epilogue_truth as E

TERMS = ("depth_normal", "distortion", "depth", "normal", "alpha")


def terms_torch(raster, world_view, W, H, FoVx, FoVy, alpha_weight=False, depth_target=None, normal_target=None, alpha_target=None,
                mask=None):
    """The five per-pixel terms [5, H, W] of one frame: raster [9, H, W] in any floating dtype (the arithmetic's), targets and mask cast
    to it. ``alpha_weight``: False, True (w = raster[7], detached) or a weight map [H, W] used as given."""
    dtype = raster.dtype
    cast = lambda t: None if t is None else t.to(dtype)
    depth_target, normal_target, alpha_target, mask = cast(depth_target), cast(normal_target), cast(alpha_target), cast(mask)
    nw, dn = E.epilogue_torch(raster, world_view, W, H, FoVx, FoVy)
    zero = torch.zeros((H, W), dtype=dtype)
    m = torch.ones((H, W), dtype=dtype) if mask is None else mask
    if torch.is_tensor(alpha_weight):          # the weight map itself, held fixed (finite differences must not move it)
        w = alpha_weight.to(dtype)
    else:
        w = raster[7].detach() if alpha_weight else torch.ones((H, W), dtype=dtype)
    t0 = w * (1 - (nw * dn).sum(0))
    t1 = raster[8]
    t2 = zero if depth_target is None else m * (raster[6] - depth_target).abs()
    if normal_target is None:
        t3 = zero
    else:
        nhat = torch.nn.functional.normalize(raster[3:6], p=2, dim=0)
        t3 = m * (1 - (nhat * normal_target).sum(0))
    t4 = zero if alpha_target is None else (raster[7] - alpha_target).abs()
    return torch.stack([t0, t1, t2, t3, t4])


def make_fixture(F, H, W, seed=0):
    """``epilogue_truth.make_fixture`` plus what the loss terms read: alpha in [0, 1], a ~70 % mask, seeded depth, unit-normal and
    binary-alpha targets, and distinct ``frame_weights`` [F, 5] (magnitudes in 0.25 .. 1.25, seeded signs). float32, on the CPU."""
    f = E.make_fixture(F, H, W, seed)
    gen = torch.Generator().manual_seed(4242 + seed)
    f["raster"][:, 7] = torch.rand(F, H, W, generator=gen)
    f["mask"] = (torch.rand(F, H, W, generator=gen) < 0.7).float()
    f["depth_target"] = f["raster"][:, 6] + 0.2 * torch.randn(F, H, W, generator=gen)
    f["normal_target"] = torch.nn.functional.normalize(torch.randn(F, 3, H, W, generator=gen), dim=1).contiguous()
    f["alpha_target"] = (torch.rand(F, H, W, generator=gen) < 0.5).float()
    sign = torch.where(torch.rand(F, 5, generator=gen) < 0.5, -1.0, 1.0)
    f["frame_weights"] = sign * (0.25 + torch.rand(F, 5, generator=gen))
    return f


def _targets(f, v, skip=()):
    pick = lambda name: None if (name in skip or f.get(name) is None) else f[name][v]
    return dict(depth_target=pick("depth_target"), normal_target=pick("normal_target"), alpha_target=pick("alpha_target"), mask=pick("mask"))


def per_pixel(f, dtype, alpha_weight=False, skip=()):
    """The restatement's per-pixel terms [F, 5, H, W] in ``dtype``. ``skip``: names among depth_target / normal_target / alpha_target /
    mask to leave out (None)."""
    with torch.no_grad():
        return torch.stack([terms_torch(f["raster"][v].to(dtype), f["world_view"][v], f["W"], f["H"], f["FoVx"], f["FoVy"], alpha_weight,
                                        **_targets(f, v, skip)) for v in range(f["raster"].shape[0])])


def grads(f, dtype, alpha_weight=False, skip=(), frame_weights=None):
    """dL/draster [F, 9, H, W] (``dtype``) of L = sum_f sum_k frame_weights[f, k] sum_p term_k(f, p) through the restatement."""
    fw = f["frame_weights"] if frame_weights is None else frame_weights
    out = []
    for v in range(f["raster"].shape[0]):
        r = f["raster"][v].to(dtype).requires_grad_()
        t = terms_torch(r, f["world_view"][v], f["W"], f["H"], f["FoVx"], f["FoVy"], alpha_weight, **_targets(f, v, skip))
        loss = (t.sum((1, 2)) * fw[v].to(dtype)).sum()
        out.append(torch.autograd.grad(loss, r)[0])
    return torch.stack(out)


def sum_bounds(t32, t64):
    """(s64 [F, 5] float64, bound [F, 5]) of the rule above from the per-pixel terms in both precisions."""
    t64 = t64.double()
    n = t64.shape[-1] * t64.shape[-2]
    s64 = t64.sum((2, 3))
    bound = 4 * (t32.double() - t64).abs().sum((2, 3)) + n * 2.0 ** -24 * t64.abs().sum((2, 3))
    return s64, bound


def check_sums(got, t32, t64, label=""):
    """Prints every (frame, term) figure, then asserts the rule. A term that is identically zero in float64 must be exactly zero."""
    got = got.detach().double().cpu()
    s64, bound = sum_bounds(t32, t64)
    bad = []
    for fr in range(s64.shape[0]):
        for k, name in enumerate(TERMS):
            err = abs(float(got[fr, k]) - float(s64[fr, k]))
            print(f"{label} frame {fr} {name:12s} s64 {float(s64[fr, k]):+.6e}  kernel err {err:.3e}  bound {float(bound[fr, k]):.3e}")
            if not err <= float(bound[fr, k]):
                bad.append((fr, name, err, float(bound[fr, k])))
    assert not bad, (label, bad)

