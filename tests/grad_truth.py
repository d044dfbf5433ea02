"""float64 autograd ground truth for the per-Gaussian stage of the backward pass (test infrastructure).

The reference's computeView2Gaussian_backward (backward.cu:381-587) and SH backward (:20-139) are the plain chain
rule of  view2gaussian(mean, scale, rot; view)  and  colour(mean, sh; campos).  In float32 they are dominated by
cancellation noise (the reference's own run-to-run spread on dL/dscale is 0.35-0.45 of the maximum), so
parity of dmean3D / drot / dscale is asserted as "error against this fp64 truth <= the oracle's own error".

The compositing stage has its own truth below (compositing_truth_arrays): autograd of the blending recurrence on a state given as
arrays, all nine cotangent planes, in float64 (the truth) or float32 (the yardstick of DESIGN.md section 4)."""
import numpy as np
import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def view2gaussian64(means, scales, rots, view):
    """[P,10] in float64; view = viewmatrix tensor [4,4] (row-vector convention)."""
    r, x, y, z = rots.unbind(-1)
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
        torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
        torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)     # gaussian -> world
    Wr = view[:3, :3].T
    Rgv = Wr @ R                                              # gaussian -> view rotation
    tg = means @ view[:3, :3] + view[3, :3]                   # view-space mean
    t2 = -(Rgv.transpose(1, 2) @ tg.unsqueeze(-1)).squeeze(-1)
    S = 1.0 / (scales * scales + 1e-7)
    C = (t2 * t2 * S).sum(-1)
    Sigma = Rgv @ torch.diag_embed(S) @ Rgv.transpose(1, 2)
    B = (Rgv @ (S * t2).unsqueeze(-1)).squeeze(-1)
    return torch.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2], Sigma[:, 2, 2],
                        B[:, 0], B[:, 1], B[:, 2], C], -1)


def colour64(means, shs, campos, deg):
    d = means - campos
    d = d / d.norm(dim=-1, keepdim=True)
    res = SH_C0 * shs[:, 0]
    if deg > 0:
        x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        res = res - SH_C1 * y * shs[:, 1] + SH_C1 * z * shs[:, 2] - SH_C1 * x * shs[:, 3]
    if deg > 1:       # real spherical harmonics of degree 2 and 3 in the 3DGS basis (forward.cu:40-66)
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = res + SH_C2[0] * xy * shs[:, 4] + SH_C2[1] * yz * shs[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * shs[:, 6] \
            + SH_C2[3] * xz * shs[:, 7] + SH_C2[4] * (xx - yy) * shs[:, 8]
        if deg > 2:
            res = res + SH_C3[0] * y * (3 * xx - yy) * shs[:, 9] + SH_C3[1] * xy * z * shs[:, 10] \
                + SH_C3[2] * y * (4 * zz - xx - yy) * shs[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * shs[:, 12] \
                + SH_C3[4] * x * (4 * zz - xx - yy) * shs[:, 13] + SH_C3[5] * z * (xx - yy) * shs[:, 14] \
                + SH_C3[6] * x * (xx - 3 * yy) * shs[:, 15]
    return torch.clamp_min(res + 0.5, 0.0)


def per_gaussian_truth(scene, view_idx, radii, dL_dv2g, dL_dcolor):
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    means = t64(scene["means3D"]).requires_grad_(True)
    scales = t64(scene["scales"]).requires_grad_(True)
    rots = t64(scene["rotations"]).requires_grad_(True)
    view = t64(scene["viewmatrix"][view_idx])
    vis = torch.tensor(np.asarray(radii) > 0)
    L = (view2gaussian64(means, scales, rots, view) * t64(dL_dv2g))[vis].sum()
    shs = None
    if scene["shs"] is not None:
        shs = t64(scene["shs"]).requires_grad_(True)
        col = colour64(means, shs, t64(scene["campos"][view_idx]), scene["sh_degree"])
        L = L + (col * t64(dL_dcolor))[vis].sum()
    L.backward()
    return dict(dL_dmean3D=means.grad.numpy(), dL_dscale=scales.grad.numpy(), dL_drot=rots.grad.numpy(),
                dL_dsh=None if shs is None else shs.grad.numpy())


def _views_chain(scene, views, radii, dL_dv2g, dL_dcolor, n_sets, magnitude):
    """The float64 chain rule of the listed views, summed (magnitude False), or the sum of the absolute values of its single-input
    parts (magnitude True: one backward pass per column of dL_dv2g, one for the colour path)."""
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    views = list(views)
    V = len(views)
    radii = np.asarray(radii).reshape(V, -1)
    P, vps = radii.shape[1], V // n_sets
    assert vps * n_sets == V and scene["means3D"].shape[0] == n_sets * P
    dL_dv2g, dL_dcolor = np.asarray(dL_dv2g).reshape(V, P, 10), np.asarray(dL_dcolor).reshape(V, P, 3)
    out = dict(dL_dmean3D=np.zeros((n_sets * P, 3)), dL_dscale=np.zeros((n_sets * P, 3)), dL_drot=np.zeros((n_sets * P, 4)),
               dL_dsh=None if scene["shs"] is None else np.zeros(tuple(scene["shs"].shape)))
    fold = (lambda g: g.abs().numpy()) if magnitude else (lambda g: g.numpy())
    for i, vi in enumerate(views):
        rows = slice((i // vps) * P, (i // vps + 1) * P)            # the Gaussians of this view's set
        means = t64(scene["means3D"][rows]).requires_grad_(True)
        scales = t64(scene["scales"][rows]).requires_grad_(True)
        rots = t64(scene["rotations"][rows]).requires_grad_(True)
        vis = torch.tensor(radii[i] > 0)                            # the kernel's  if (!(radii[idx] > 0)) continue
        prod = view2gaussian64(means, scales, rots, t64(scene["viewmatrix"][vi])) * t64(dL_dv2g[i])
        losses = [prod[:, c][vis].sum() for c in range(10)] if magnitude else [prod[vis].sum()]
        for L in losses:
            grads = torch.autograd.grad(L, (means, scales, rots), retain_graph=True, allow_unused=True)
            for k, g in zip(("dL_dmean3D", "dL_dscale", "dL_drot"), grads):
                if g is not None:       # (columns 0..5 are the gradient of Sigma, which does not depend on the mean)
                    out[k][rows] += fold(g)
        if scene["shs"] is not None:
            shs = t64(scene["shs"][rows]).requires_grad_(True)
            col = colour64(means, shs, t64(scene["campos"][vi]), scene["sh_degree"])
            gm, gsh = torch.autograd.grad((col * t64(dL_dcolor[i]))[vis].sum(), (means, shs))
            out["dL_dmean3D"][rows] += fold(gm)
            out["dL_dsh"][rows] += fold(gsh)
    return out


def per_gaussian_truth_views(scene, views, radii, dL_dv2g, dL_dcolor, n_sets=1):
    """per_gaussian_truth summed over the listed views (indices into the scene's cameras): radii [V,P], dL_dv2g [V,P,10], dL_dcolor
    [V,P,3], row i belonging to views[i]; each view restricted to its rows with radii > 0. n_sets > 1: the Gaussian tensors are
    [n_sets * P, ...] and the views of set s are rows s * V/n_sets .. (s + 1) * V/n_sets; each set is summed over its own views only."""
    return _views_chain(scene, views, radii, dL_dv2g, dL_dcolor, n_sets, False)


def per_gaussian_term_magnitude(scene, views, radii, dL_dv2g, dL_dcolor, n_sets=1):
    """A per output element: the sum over the views and over the ten columns of dL_dv2g of |the contribution of that one column alone|
    (ten backward passes per view, the other nine columns zeroed), plus |the contribution of the colour path alone| (dL_dmean3D and
    dL_dsh). The net gradient is a strong cancellation of these parts; 2^-24 * A is the scale of ONE float32 rounding of them."""
    return _views_chain(scene, views, radii, dL_dv2g, dL_dcolor, n_sets, True)


NEAR_PLANE, FAR_PLANE = 0.2, 100.0
GUARD_REL = 1e-5        # a pair whose alpha * 255 or t / NEAR_PLANE lies this close to 1 may be classified differently in float32
T_AGREE = 1e-3          # the truth's final transmittance against the state's: one entry blended or not moves it by >= 3.9e-3


def compositing_truth_arrays(view2gaussian, opacity, colour, point_list, ranges, n_contrib, W, H, tanfovx, tanfovy, weights, bg=None,
                             dtype=np.float64, final_T=None):
    """Autograd of the compositing stage on a STATE given as arrays -- the oracle's intermediates or what helpers.run_hip exports from
    a HIP workspace: view2gaussian [P,10], opacity * coef [P], colour [P,3], point_list (Gaussian ids), ranges [tiles,2] into it,
    n_contrib [2,H,W] (0: entries of the tile list the pixel visited up to its last blended one; 1: the 1-based list position of the
    median contributor, 0xFFFFFFFF for none), bg [3] or None.

    weights: one [9,H,W] cotangent or a list of them; the loss of each is  sum_pixels sum_ch weights[ch] * value[ch]  with
      ch 0..2  colour, background term T_final * bg included;
      ch 3..5  the blended unit normal;
      ch 6     t of the entry at list position n_contrib[1] - 1 if that entry is blended (no median: 0);
      ch 7     nothing: the reference's backward never reads the alpha cotangent;
      ch 8     A * D2 - D1^2  with  A = sum w, D1 = sum w m, D2 = sum w m^2  over the pixel's blended entries, w = alpha * T DETACHED,
               m = (FAR t - FAR NEAR) / ((FAR - NEAR) t): the pair distortion  sum_{i<k} w_i w_k (m_i - m_k)^2  NOT normalised by
               (1 - T)^2 + 1e-7, the weights constants. Its d/dm_k = 2 w_k (m_k A - D1) is what backward.cu:850-852 keeps.
    The lists, the list positions and the skip decisions (t > NEAR, alpha >= 1/255) are constants, as the analytic backward assumes;
    they are always decided in float64, whatever `dtype`. A pair within GUARD_REL of a threshold is one float64 cannot decide for a
    float32 state: with `final_T` (the state's own final transmittance [H,W]) such a pair is blended or not as that plane says; one
    that stays undecided (no final_T, or no clear answer) has its Gaussian listed in guard_ids.

    dtype float64 is the truth. float32 is the yardstick: the same function with float32 leaves and float32 arithmetic, the ray
    intersection (t, the exponent) in double from float32 operands as forward.cu:462-475 declares it. Gradients come back float64
    (sums over the tiles of a Gaussian are added in float64 in either mode).

    Returns a dict (a list of dicts for a list of weights) with dL_dopacity [P], dL_dcolor [P,3], dL_dview2gaussian [P,10], and
      value [9,H,W]     the float64/float32 forward: ch 0..6 as above, ch 7 = A, ch 8 = the ATTACHED, NORMALISED distortion
                        (A D2 - D1^2) / ((1 - T)^2 + 1e-7), i.e. what the forward's plane 8 holds;
      median_id [H,W]   the Gaussian id of the blended median contributor, -1 for none;
      T_final [H,W]     the transmittance behind the last blended entry (to be held against the state's: T_AGREE);
      pairs, guard_pairs, guard_resolved, guard_ids   the number of in-range (pixel, entry) pairs, of those within GUARD_REL of a skip
                        threshold, of those decided by final_T, and the Gaussians of the undecided ones (to be left out: none allowed)."""
    single = not isinstance(weights, (list, tuple))
    wlist = [weights] if single else list(weights)
    td = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=td)
    v2g_all, opac_all, col_all = tt(view2gaussian), tt(opacity).reshape(-1), tt(colour)
    P = v2g_all.shape[0]
    wts = [torch.tensor(np.asarray(w, dtype=np.float64)).to(td) for w in wlist]
    bgt = torch.zeros(3, dtype=td) if bg is None else tt(np.asarray(bg).reshape(-1)[:3])
    focal_x = np.float32(W) / (np.float32(2.0) * np.float32(tanfovx))
    focal_y = np.float32(H) / (np.float32(2.0) * np.float32(tanfovy))
    n_contrib = np.asarray(n_contrib).astype(np.int64) & 0xFFFFFFFF
    last = torch.tensor(n_contrib[0])
    median = torch.tensor(np.where(n_contrib[1] == 0xFFFFFFFF, 0, n_contrib[1]) - 1)       # 0-based list position, -1: none
    ranges, point_list = np.asarray(ranges).astype(np.int64), np.asarray(point_list).astype(np.int64)
    gx = (W + 15) // 16
    grads = [dict(dL_dopacity=np.zeros(P), dL_dcolor=np.zeros((P, 3)), dL_dview2gaussian=np.zeros((P, 10))) for _ in wlist]
    value = np.zeros((9, H, W))
    median_id = np.full((H, W), -1, np.int64)
    T_plane = np.ones((H, W))
    final_T = None if final_T is None else np.asarray(final_T, np.float64).reshape(H, W)
    pairs = guard_pairs = guard_resolved = 0
    guard_ids = set()
    for tile in range(ranges.shape[0]):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        if r1 <= r0:
            continue
        ty, tx = divmod(tile, gx)
        ys, xs = torch.meshgrid(torch.arange(ty * 16, min(ty * 16 + 16, H)), torch.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        r1 = min(r1, r0 + int(last[ys, xs].max()))                  # no pixel of the tile went further down the list
        if r1 <= r0:
            continue
        ids_np = point_list[r0:r1]
        ids = torch.tensor(ids_np)
        # the ray is rounded to float32 in the reference (forward.cu:448); keep that rounding, the exponent amplifies it
        rx = ((xs.double() + 0.5 - W / 2.) / float(focal_x)).float().to(td).unsqueeze(1)
        ry = ((ys.double() + 0.5 - H / 2.) / float(focal_y)).float().to(td).unsqueeze(1)
        v_leaf = v2g_all[ids].clone().requires_grad_(True)
        o_leaf = opac_all[ids].clone().requires_grad_(True)
        c_leaf = col_all[ids].clone().requires_grad_(True)
        v = v_leaf.unsqueeze(0)                                     # [1,n,10]
        n0 = v[..., 0] * rx + v[..., 1] * ry + v[..., 2]
        n1 = v[..., 1] * rx + v[..., 3] * ry + v[..., 4]
        n2 = v[..., 2] * rx + v[..., 4] * ry + v[..., 5]
        AA = (rx * n0 + ry * n1 + n2).double()
        BB = (2 * (v[..., 6] * rx + v[..., 7] * ry + v[..., 8])).double()
        t = (-BB / (2 * AA)).to(td)
        power = (-0.5 * (-(BB / AA) * (BB / 4.) + v[..., 9].double())).to(td)
        # C - B^2 / A is the minimum of a positive semi-definite form: power > 0 is roundoff (a ray through the Gaussian's centre, where
        # two numbers of 1e3 cancel) and differs between two evaluations. The clamp is a value fix-up, not a branch of the derivative:
        # backward.cu differentiates through it, and so does this (a clamped pair would otherwise lose its whole gradient in one
        # evaluation and keep it in the other: 0.3 of a row's maximum on fixture D, tests/channel_cases.py)
        power = power + (torch.clamp_max(power, 0.0) - power).detach()
        raw =o_leaf.unsqueeze(0) * torch.exp(power)
        alpha = torch.clamp_max(raw, 0.99)
        pos = torch.arange(len(ids)).unsqueeze(0)
        with torch.no_grad():
            # the decisions, in float64 from the same operands in either mode
            v64, rx64, ry64 = v2g_all[ids].double().unsqueeze(0), rx.double(), ry.double()
            m0 = v64[..., 0] * rx64 + v64[..., 1] * ry64 + v64[..., 2]
            m1 = v64[..., 1] * rx64 + v64[..., 3] * ry64 + v64[..., 4]
            m2 = v64[..., 2] * rx64 + v64[..., 4] * ry64 + v64[..., 5]
            A64 = rx64 * m0 + ry64 * m1 + m2
            B64 = 2 * (v64[..., 6] * rx64 + v64[..., 7] * ry64 + v64[..., 8])
            t64_ = -B64 / (2 * A64)
            raw64 = opac_all[ids].double().unsqueeze(0) * torch.exp(torch.clamp_max(-0.5 * (-(B64 / A64) * (B64 / 4.) + v64[..., 9]), 0.0))
            in_range = pos < last[ys, xs].unsqueeze(1)
            ok_t, ok_a = t64_ > NEAR_PLANE, raw64 >= 1.0 / 255.0
            near_t, near_a = (t64_ / NEAR_PLANE - 1.0).abs() <= GUARD_REL, (raw64 * 255.0 - 1.0).abs() <= GUARD_REL
            mask = ok_t & ok_a & in_range
            near = in_range & (near_t | near_a) & (ok_t | near_t) & (ok_a | near_a)         # float64 cannot speak for the state here
            pairs += int(in_range.sum())
            guard_pairs += int(near.sum())
            if near.any() and final_T is not None:
                # ... so the state speaks: of the 2^k ways to blend a pixel's k guarded entries, the one whose transmittance
                # prod(1 - alpha) is the state's own final T (a blended entry moves it by at least 1/255 = 3.9e-3, float32 by 1e-6)
                a64 = torch.clamp_max(raw64, 0.99)
                for p in torch.nonzero(near.any(1)).reshape(-1).tolist():
                    ks = torch.nonzero(near[p]).reshape(-1).tolist()
                    want = float(final_T[int(ys[p]), int(xs[p])])
                    cands = []
                    for bits in range(1 << len(ks)) if len(ks) <= 4 else ():
                        mrow = mask[p].clone()
                        for i, k in enumerate(ks):
                            mrow[k] = bool(bits >> i & 1)
                        cands.append((abs(float(torch.prod(1 - a64[p] * mrow)) / want - 1.0), bits, mrow))
                    cands.sort(key=lambda c: c[0])
                    if cands and cands[0][0] <= T_AGREE and cands[1][0] > 2 * T_AGREE:
                        mask[p] = cands[0][2]
                        guard_resolved += len(ks)
                    else:
                        guard_ids.update(ids_np[ks].tolist())
            elif near.any():
                guard_ids.update(ids_np[near.any(0).numpy()].tolist())
        one = torch.ones((), dtype=td)
        a = torch.where(mask, alpha, 0 * one)
        T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), 1 - a[:, :-1]], 1), 1)
        T_final = T[:, -1] * (1 - a[:, -1])
        wgt = a * T
        length = torch.sqrt(n0 * n0 + n1 * n1 + n2 * n2 + 1e-7)
        ts = torch.where(mask, t, one)                              # (entries that are not blended may have any t, 0 included)
        mp = median[ys, xs]
        has = mp >= 0
        mpc = mp.clamp(0, len(ids) - 1).unsqueeze(1)
        has = has & (mp < len(ids)) & mask.gather(1, mpc).squeeze(1)
        med_t = torch.where(has, ts.gather(1, mpc).squeeze(1), 0 * one)
        w_det = wgt.detach()
        m = (FAR_PLANE * ts - FAR_PLANE * NEAR_PLANE) / ((FAR_PLANE - NEAR_PLANE) * ts)
        A_, D1, D2 = w_det.sum(1), (w_det * m).sum(1), (w_det * m * m).sum(1)
        chans = [wgt @ c_leaf[:, 0] + T_final * bgt[0], wgt @ c_leaf[:, 1] + T_final * bgt[1], wgt @ c_leaf[:, 2] + T_final * bgt[2],
                 (wgt * (-n0 / length)).sum(1), (wgt * (-n1 / length)).sum(1), (wgt * (-n2 / length)).sum(1),
                 med_t, None, A_ * D2 - D1 * D1]
        with torch.no_grad():
            for ch in (0, 1, 2, 3, 4, 5, 6):
                value[ch, ys, xs] = chans[ch].double().numpy()
            Aw, E1, E2 = wgt.sum(1), (wgt * m).sum(1), (wgt * m * m).sum(1)
            value[7, ys, xs] = Aw.double().numpy()
            T_plane[ys, xs] = T_final.double().numpy()
            value[8, ys, xs] = ((Aw * E2 - E1 * E1) / ((1 - T_final) * (1 - T_final) + 1e-7)).double().numpy()
            median_id[ys, xs] = torch.where(has, ids[mpc.squeeze(1)], torch.full_like(mp, -1)).numpy()
        for g, w in zip(grads, wts):
            loss = sum((chans[ch] * w[ch, ys, xs]).sum() for ch in (0, 1, 2, 3, 4, 5, 6, 8))
            gv, go, gc = torch.autograd.grad(loss, (v_leaf, o_leaf, c_leaf), retain_graph=True, allow_unused=True)
            for key, gt in (("dL_dview2gaussian", gv), ("dL_dopacity", go), ("dL_dcolor", gc)):
                if gt is not None:
                    np.add.at(g[key], ids_np, gt.double().numpy())
    for g in grads:
        g.update(value=value, median_id=median_id, T_final=T_plane, pairs=pairs, guard_pairs=guard_pairs, guard_resolved=guard_resolved,
                 guard_ids=sorted(guard_ids))
    return grads[0] if single else grads


def compositing_truth(scene, o, weights, view_idx=0, dtype=np.float64):
    """compositing_truth_arrays on the oracle's intermediates `o` of one view of `scene` (helpers.run_oracle): float64 autograd of the
    compositing stage for the loss  sum(weights * out)  over all nine planes. Returns gradients w.r.t. the per-Gaussian compositing
    inputs: opacity*coef [P], colour [P,3], view2gaussian [P,10] (and the forward values and guard counts documented there)."""
    col = o["rgb"] if scene["colors_precomp"] is None else scene["colors_precomp"]
    col = col.detach().cpu().numpy() if torch.is_tensor(col) else col
    bg = scene["bg"].detach().cpu().numpy() if torch.is_tensor(scene["bg"]) else scene["bg"]
    return compositing_truth_arrays(o["view2gaussian"], o["conic_opacity"][:, 3], col, o["point_list"], o["ranges"], o["n_contrib"],
                                    scene["W"], scene["H"], scene["tanfovx"], scene["tanfovy"], weights, bg=bg, dtype=dtype,
                                    final_T=o["final_T"][0] if "final_T" in o else None)
