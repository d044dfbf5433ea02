"""Cycle-aggregation loop and orbit rendering of the inference path (reference visualize.py:221-416), batched.

Reference shape of the work per batch of B images (visualize.py):
  :283       predict Gaussians of the input image from the canonical camera          (B x 65,536 Gaussians)
  :293-314   render them from 8 orbit cameras: 8 x B separate rasterizer calls, each with a host sync and .cpu()
  :326-340   feed every render (clamped RGB + alpha, rendered median depth) back through the predictor with ITS camera
             and torch.cat the 9 Gaussian sets per key                              (B x 589,824 Gaussians)
  :387-416   render the merged set along a 128-view orbit: 128 x B rasterizer calls
MI355X shape of the same work here:
  * the 8 novel views of ALL B images are ONE launch sequence (f3dg_forward_sets: B Gaussian sets x 8 cameras, ~20 kernel
    launches per batch instead of per (image, view)); the 128 orbit cameras of an image go through one launch sequence per
    chunk of views (render_views); nothing leaves the GPU;
  * one kernel (f3dg_cycle_inputs) turns the rendered rasters into the next predictor inputs -- clamp(rgb) || alpha and
    the median depth, view-major so that the B inputs of a novel view are one contiguous predictor batch;
  * the 8 re-predictions are 8 predictor calls of B images each, as in the reference (visualize.py:326-340), and the splat
    head writes every pass directly into the preallocated merged buffers (no torch.cat chain, no O(n^2) re-copies);
  * the order of the merged set is the reference's: canonical view first, then orbit views 0..7;
  * ``cycle_aggregate(differentiable=True)`` is the same loop under autograd, for training through the aggregation: the hand-off kernel
    has an adjoint (f3dg_cycle_inputs_backward) and the merge is one node over the splat head's backward (``splat_head_merge``).
"""
import torch

from . import cameras
from .gaussian_predictor import GAUSSIAN_KEYS, allocate_gaussians, splat_head, splat_head_merge
from .gaussian_renderer import cycle_inputs, render_views


def cycle_aggregate(model, images, depth, cfg, rig=None, num_views=8, yaw_diff=0.25, pitch_diff=0.15,
                    return_renders=False, differentiable=False, grad_through_renders=True):
    """images [B,3,H,W] in [0,1], depth [B,1,H,W] (z in camera space). Returns the merged Gaussian dict
    (every value [B, (1+num_views)*H*W, ...]) -- what visualize.py calls ``gaussian_splat_batch_merge``.

    ``differentiable=True`` (with grad mode on; under ``torch.no_grad()`` it is the inference call): the merged set carries the autograd
    graph back through all 1 + num_views predictor passes -- and, with ``grad_through_renders`` (default), through the hand-off and the
    novel-view renders into pass 0 as well; ``grad_through_renders=False`` detaches the re-prediction inputs, so that the renders are
    data and only the predictor passes are trained. The training shape:

        merged = cycle_aggregate(model, images, depth, cfg, differentiable=True)
        out = render_views(merged, None, world_views, full_projs, centers, bg, cfg, differentiable=True)
        losses.photometric_loss(out["render"], target).backward()

    The novel views are rendered on a workspace of their own, in all nine channels and the reference arithmetic (what the differentiable
    render requires), so a later differentiable render of the merged set does not invalidate their backward."""
    if differentiable and torch.is_grad_enabled():
        return _cycle_aggregate_autograd(model, images, depth, cfg, rig, num_views, yaw_diff, pitch_diff, return_renders,
                                         grad_through_renders)
    with torch.no_grad():
        return _cycle_aggregate_inference(model, images, depth, cfg, rig, num_views, yaw_diff, pitch_diff, return_renders)


def _cycle_aggregate_inference(model, images, depth, cfg, rig, num_views, yaw_diff, pitch_diff, return_renders):
    device = images.device
    B, _, H, W = images.shape
    HW = H * W
    rig = rig or cameras.OrbitRig(cfg)
    cano = rig.canonical
    orbit = rig.orbit(num_views, yaw_diff, pitch_diff)
    background = torch.zeros(3, dtype=torch.float32, device=device)
    squre_clip = cfg['opt']['squre_clip']

    merged = allocate_gaussians(B, (1 + num_views) * HW, device)

    # first forward: input image + alpha 1, canonical camera (visualize.py:282-283)
    x0 = torch.cat([images, torch.ones_like(images[:, :1])], 1).unsqueeze(1)
    v2w0 = cano.view_to_world_transforms.reshape(1, 1, 4, 4).expand(B, 1, 4, 4).to(device)
    q0 = cano.source_cv2wT_quat.reshape(1, 1, 4).expand(B, 1, 4).to(device)
    model(x0, background, v2w0, q0, return_3d_features=True, render=False, squre_clip=squre_clip, unet_depth=depth,
          out=merged, n_offset=0)
    first = {k: merged[k][:, :HW] for k in GAUSSIAN_KEYS}

    # 8 novel views of every image: one launch sequence for the whole batch (visualize.py:293-314), then the hand-off kernel
    wv, fp, cc = (orbit.world_view_transforms.to(device), orbit.full_proj_transforms.to(device),
                  orbit.camera_centers.to(device))
    # (the hand-off consumes RGB, alpha and the median depth only -- visualize.py:304-306 -- so the compositing kernel is asked for
    # just those: no normal / distortion accumulators, 16 B per pixel less written)
    r = render_views(first, None, wv, fp, cc, background, cfg, epilogue=False, channels="rgb_depth_alpha")
    xin, zmed = cycle_inputs(r["raster"], B, num_views)        # [V,B,4,H,W] = clamp(rgb) || alpha (visualize.py:311,332), [V,B,1,H,W]

    # re-predict from every novel view with its own camera and merge in place (visualize.py:326-340)
    v2w = orbit.view_to_world_transforms.to(device)       # [V,1,4,4]
    quat = orbit.source_cv2wT_quat.to(device)              # [V,1,4]
    for v in range(num_views):
        model(xin[v].unsqueeze(1), background, v2w[v:v + 1].expand(B, 1, 4, 4), quat[v:v + 1].expand(B, 1, 4),
              return_3d_features=True, render=False, squre_clip=squre_clip, unet_depth=zmed[v],
              out=merged, n_offset=(1 + v) * HW)
    if return_renders:
        xb = xin.transpose(0, 1)                           # [B,V,4,H,W]
        return merged, dict(rgb=xb[:, :, :3], alpha=xb[:, :, 3:4], depth=zmed.transpose(0, 1))
    return merged


def _cycle_aggregate_autograd(model, images, depth, cfg, rig, num_views, yaw_diff, pitch_diff, return_renders, grad_through_renders):
    """The same loop with every stage under autograd: the predictor passes stop before the head (``head=False``), the first set goes
    through ``splat_head``, the batched differentiable render and the hand-off kernel with its adjoint, and ONE ``splat_head_merge``
    node builds the merged set from the 1 + num_views passes (pass 0's head is recomputed into the merged buffer: 192 B per Gaussian,
    and autograd sums the two contributions to its ``net_out``)."""
    device = images.device
    B = images.shape[0]
    rig = rig or cameras.OrbitRig(cfg)
    cano = rig.canonical
    orbit = rig.orbit(num_views, yaw_diff, pitch_diff)
    background = torch.zeros(3, dtype=torch.float32, device=device)
    squre_clip = cfg['opt']['squre_clip']
    ray_dirs = model.gaussian_predictor.ray_dirs

    x0 = torch.cat([images, torch.ones_like(images[:, :1])], 1).unsqueeze(1)
    v2w0 = cano.view_to_world_transforms.reshape(1, 1, 4, 4).expand(B, 1, 4, 4).to(device)
    q0 = cano.source_cv2wT_quat.reshape(1, 1, 4).expand(B, 1, 4).to(device)
    net0, depth0 = model(x0, background, v2w0, q0, return_3d_features=True, render=False, squre_clip=squre_clip, unet_depth=depth,
                         head=False)
    nets, depths, v2ws, quats = [net0], [depth0], [v2w0.reshape(B, 4, 4)], [q0.reshape(B, 4)]
    first = splat_head(net0, depth0, ray_dirs, v2ws[0], quats[0], squre_clip)

    wv, fp, cc = (orbit.world_view_transforms.to(device), orbit.full_proj_transforms.to(device),
                  orbit.camera_centers.to(device))
    # (workspace=None: a workspace of this call's own, which no later forward can make stale before backward() reads it)
    r = render_views(first, None, wv, fp, cc, background, cfg, epilogue=False, differentiable=True)
    xin, zmed = cycle_inputs(r["raster"], B, num_views)
    if not grad_through_renders:
        xin, zmed = xin.detach(), zmed.detach()

    v2w = orbit.view_to_world_transforms.to(device)
    quat = orbit.source_cv2wT_quat.to(device)
    for v in range(num_views):
        net_v, depth_v = model(xin[v].unsqueeze(1), background, v2w[v:v + 1].expand(B, 1, 4, 4), quat[v:v + 1].expand(B, 1, 4),
                               return_3d_features=True, render=False, squre_clip=squre_clip, unet_depth=zmed[v], head=False)
        nets.append(net_v)
        depths.append(depth_v)
        v2ws.append(v2w[v].reshape(1, 4, 4).expand(B, 4, 4))
        quats.append(quat[v].reshape(1, 4).expand(B, 4))
    merged = splat_head_merge(nets, depths, ray_dirs, v2ws, quats, squre_clip)
    if return_renders:
        xb = xin.transpose(0, 1)
        return merged, dict(rgb=xb[:, :, :3], alpha=xb[:, :, 3:4], depth=zmed.transpose(0, 1))
    return merged


@torch.no_grad()
def render_orbit(gaussians, cfg, rig=None, num_views=128, yaw_diff=0.25, pitch_diff=0.15, views_per_call=32,
                 epilogue=True, images_per_call=1):
    """visualize.py:343-416: the frontal camera + num_views orbit cameras are built exactly as the reference does,
    and views 1..num_views are rendered. Returns dict of [B, num_views, C, H, W] tensors (render, rendered_depth,
    rendered_alpha, depth_normal). The reference's background[th:th+1] out-of-range read is NOT
    reproduced: the intended background (0,0,0) is used. ``images_per_call`` > 1 renders that many images' views in one launch
    sequence (f3dg_forward_sets); the workspace grows with images_per_call x views_per_call x Gaussians."""
    rig = rig or cameras.OrbitRig(cfg)
    cams = rig.orbit_with_frontal(num_views, yaw_diff, pitch_diff)
    device = gaussians["xyz"].device
    B = gaussians["xyz"].shape[0]
    res = int(cfg['model']['training_resolution'])
    wv = cams.world_view_transforms[1:].to(device)
    fp = cams.full_proj_transforms[1:].to(device)
    cc = cams.camera_centers[1:].to(device)
    bg = torch.zeros(3, dtype=torch.float32, device=device)
    out = {"render": torch.empty((B, num_views, 3, res, res), device=device),
           "rendered_depth": torch.empty((B, num_views, 1, res, res), device=device),
           "rendered_alpha": torch.empty((B, num_views, 1, res, res), device=device)}
    if epilogue:
        out["depth_normal"] = torch.empty((B, num_views, 3, res, res), device=device)
    workspaces = {}
    keys = ("render", "rendered_depth", "rendered_alpha") + (("depth_normal",) if epilogue else ())
    for b0 in range(0, B, max(int(images_per_call), 1)):
        b1 = min(b0 + max(int(images_per_call), 1), B)
        sub = gaussians if (b0, b1) == (0, B) else {k: v[b0:b1] for k, v in gaussians.items() if torch.is_tensor(v)}
        for a in range(0, num_views, views_per_call):
            e = min(a + views_per_call, num_views)
            one = b1 - b0 == 1
            r = render_views(gaussians if one else sub, b0 if one else None, wv[a:e], fp[a:e], cc[a:e], bg, cfg,
                             workspace=workspaces.get((b1 - b0, e - a)), epilogue=epilogue, channels="rgb_depth_alpha")
            workspaces[(b1 - b0, e - a)] = r["workspace"]
            for k in keys:
                out[k][b0:b1, a:e] = r[k].reshape((b1 - b0, e - a) + tuple(r[k].shape[1:]))
    return out
