"""Differentiable torch restatement of the cycle-aggregative projection ("splat head") -- TEST INFRASTRUCTURE ONLY.

The reference's lines, op for op (src/gaussian_predictor.py: get_pos_from_network_output :857-881, forward :961-1002, transform_rotations
:839-855 with quaternion_raw_multiply :45-64, transform_SHs :821-837 with the matrices of :649-655, flatten_vector :788-791), in the dtype
of ``net_out`` (float32 or float64) and on its device. Its float32 forward is pinned to the reference's fixtures and its float32 gradients
to the reference's own autograd (tests/test_splat_head_backward.py); its float64 autograd is the gradient truth of the backward kernel.
Its float64 forward on the call's own float32 inputs, with an error scale per element, is the truth of the forward kernel (second half).
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest", "unet_depth")
# gradient channel groups of the tolerance rule: six slices of d_net_out [B,23,H,W] and d_depth
GROUPS = {"offset": slice(0, 3), "opacity": slice(3, 4), "scaling": slice(4, 7), "rotation": slice(7, 11), "dc": slice(11, 14),
          "rest": slice(14, 23)}
V_TO_SH = ((0.0, 0.0, -1.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0))


def _flatten(x):
    return x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)


def splat_head_torch(net_out, depth, ray_dirs, v2w, quat, squre_clip=10000.0):
    dt, dev = net_out.dtype, net_out.device
    B, _, H, W = net_out.shape
    ray_dirs, v2w, quat = ray_dirs.to(dev, dt).reshape(1, 3, H, W), v2w.to(dev, dt).reshape(B, 4, 4), quat.to(dev, dt).reshape(B, 4)
    depth = depth.to(dt)
    offset, opacity, scaling, rotation, fdc, frest = net_out.split([3, 1, 3, 4, 3, 9], dim=1)
    pos = ray_dirs.expand(B, 3, H, W).clone() * depth + offset
    pos = _flatten(pos)
    pos = torch.cat([pos, torch.ones((B, pos.shape[1], 1), device=dev, dtype=dt)], dim=2)
    pos = torch.bmm(pos, v2w)
    pos = pos[:, :, :3] / (pos[:, :, 3:] + 1e-10)
    if squre_clip < 10.0:
        pos[:, :, 0].clamp_(-squre_clip, squre_clip)
        pos[:, :, 1].clamp_(-squre_clip, squre_clip)
    out = {"xyz": pos, "opacity": _flatten(torch.sigmoid(opacity)), "scaling": _flatten(torch.exp(scaling)),
           "features_dc": _flatten(fdc).unsqueeze(2), "unet_depth": _flatten(depth)}
    b = _flatten(F.normalize(rotation))
    a = quat.unsqueeze(1).expand(*b.shape)
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    out["rotation"] = torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                                   aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)
    rest = _flatten(frest)
    rest = rest.reshape(B, rest.shape[1], -1, 3)                                    # b n sh rgb
    v_to_sh = torch.tensor(V_TO_SH, dtype=dt, device=dev).unsqueeze(0).expand(B, 3, 3)
    T = torch.bmm(torch.bmm(v_to_sh.transpose(1, 2), v2w[:, :3, :3]), v_to_sh)
    shs = rest.permute(0, 1, 3, 2).reshape(B, -1, 3)                                # b (n rgb) sh
    out["features_rest"] = torch.bmm(shs, T).reshape(B, -1, 3, 3).permute(0, 1, 3, 2)
    return {k: out[k].contiguous() for k in KEYS}


def restatement_grads(inputs, cots, squre_clip, dtype, device="cpu"):
    """(d_net_out, d_depth) of sum_k <out_k, cots[k]> by the restatement's autograd in ``dtype``; ``cots[k]`` None = output unused."""
    net = inputs["net_out"].detach().to(device, dtype).requires_grad_()
    dep = inputs["depth"].detach().to(device, dtype).requires_grad_()
    out = splat_head_torch(net, dep, inputs["ray_dirs"], inputs["v2w"], inputs["quat"], squre_clip)
    used = [k for k in KEYS if cots.get(k) is not None]
    gn, gd = torch.autograd.grad([out[k] for k in used], [net, dep], [cots[k].to(device, dtype) for k in used], allow_unused=True)
    gn = torch.zeros_like(net) if gn is None else gn
    gd = torch.zeros_like(dep) if gd is None else gd
    return gn.detach(), gd.detach()


def by_group(d_net, d_depth):
    g = {name: d_net[:, sl] for name, sl in GROUPS.items()}
    g["depth"] = d_depth
    return g


def group_bounds(g32, g64):
    """Per group: (E_ref, max|g64|) with E_ref = max|g32 - g64| / max|g64| -- the float32 error of the reference's own autograd."""
    res = {}
    for name, t64 in by_group(*g64).items():
        t32 = by_group(*g32)[name]
        m = float(t64.abs().max())
        res[name] = (float((t32.double().cpu() - t64.cpu()).abs().max()) / m if m > 0 else 0.0, m)
    return res


def check_groups(got, g32, g64, factor=4.0, label="", mask=None):
    """The tolerance rule: per group max|got - g64| <= factor * E_ref * max|g64|. ``mask`` [B,1,H,W] bool: pixels that take part.
    Prints every figure before asserting; returns {group: (E_ref, kernel error relative to max|g64|)}."""
    if mask is not None:
        sel = lambda pair: tuple(torch.where(mask.to(t.device), t, torch.zeros_like(t)) for t in pair)
        got, g32, g64 = sel(got), sel(g32), sel(g64)
    bounds = group_bounds(g32, g64)
    figures, bad = {}, []
    for name, t in by_group(*got).items():
        e_ref, m = bounds[name]
        err = float((t.double().cpu() - by_group(*g64)[name].cpu()).abs().max())
        figures[name] = (e_ref, err / m if m > 0 else err)
        print(f"{label} {name:8s} E_ref {e_ref:.3e}  kernel {figures[name][1]:.3e}  max|g64| {m:.3e}")
        if not (np.isfinite(err) and err <= factor * e_ref * m):
            bad.append((name, figures[name]))
    assert not bad, (label, bad)
    return figures


def load_inputs():
    g = np.load(os.path.join(GOLD, "splat_head.npz"))
    return {k: torch.from_numpy(g[k]) for k in ("net_out", "depth", "ray_dirs", "v2w", "quat")}, g


def load_cotangents():
    g = np.load(os.path.join(GOLD, "splat_head_grad.npz"))
    return {k: torch.from_numpy(g["cot_" + k]) for k in KEYS}, g


# ------------------------------------------------------------------------------------------------ the forward against float64
# ("the splat head's forward against float64"; figure and bars: tests/forward_bars.py)
K_GROUPS = ("xyz", "opacity", "scaling", "rotation", "features_rest")      # features_dc and unet_depth are copies: bit-equal
_HAMILTON = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0))       # rotation_k = sum_i +-a_i * b_[_HAMILTON[k][i]]
OPACITY_LOGITS = (-110.0, -90.0, -88.0, -20.0, 0.0, 20.0, 90.0, 110.0)
SCALING_LOGITS = (-104.0, -88.0, -87.0, 0.0, 88.0, 89.0)
QUAT_NORMS = (0.0, 1e-20, 1e-13, 1e-11, 1.0, 1e3)                           # clear of F.normalize's 1e-12 clamp itself
# float32 roundings on the longest chain to an element of the group, each at most 2^-24 of the scale (exp and sigmoid: one ulp = 2):
# the a-priori bound of K for ANY correct float32 evaluation, to first order -- what the restatement is held to on the host
#   xyz       p: 2; a row of [p,1] @ M: 1 product + 3 additions -> 6 for w_j and for w_3, + 1e-10: 1, the division: 1
#   opacity   exp 2, 1 + e, 1 / (.)
#   scaling   exp 2
#   rotation  |q|^2: 1 + 3, halved by the root, root 1, division 1 -> 4 on b^; product 1, three additions
#   rest      products 1, two additions (T's entries are signed copies of M's)
OP_COUNT = {"xyz": 14.0, "opacity": 4.0, "scaling": 2.0, "rotation": 8.0, "features_rest": 3.0}


def forward_truth(inputs, squre_clip=10000.0):
    """The float64 forward on the call's own float32 inputs, with the error scale A of every element and the clamp's classes.

    Returns {"out": {key: float64}, "A": {group: float64, shaped like the output}, "clamped": bool [B,n,3] (x / y beyond the clip:
    the result is +-float32(squre_clip) to the bit), "fragile": bool [B,n,3] (x / y within 2^-18 of the clip: in no bar and no exactness
    rule), "den": [B,n,1]}. ``out["xyz"]`` is the position BEFORE the clamp; the clamped elements are held by the exactness rule."""
    f = lambda k: inputs[k].detach().cpu().double()
    net, depth, rd, M, qc = f("net_out"), f("depth"), f("ray_dirs"), f("v2w"), f("quat")
    B, _, H, W = net.shape
    HW = H * W
    with torch.no_grad():
        out = splat_head_torch(net, depth, rd, M, qc, 10000.0)
    M, qc, rd = M.reshape(B, 4, 4), qc.reshape(B, 4), rd.reshape(1, 3, HW)
    d, off = depth.reshape(B, 1, HW), net[:, :3].reshape(B, 3, HW)
    p = rd * d + off
    a = (rd * d).abs() + off.abs()                                                             # pos: |ray d| + |offset|
    Aw = torch.einsum("bin,bij->bnj", a + p.abs(), M[:, :3].abs()) + M[:, 3].abs().unsqueeze(1)      # the row vector [p,1] @ M
    den = torch.einsum("bin,bi->bn", p, M[:, :3, 3]).unsqueeze(-1) + M[:, 3, 3].reshape(B, 1, 1) + 1e-10
    X = out["xyz"]
    A = {"xyz": (Aw[..., :3] + X.abs() * Aw[..., 3:]) / den.abs() + X.abs(),
         "opacity": out["opacity"].abs(), "scaling": out["scaling"].abs()}
    bh = _flatten(F.normalize(net[:, 7:11]))                                                   # B,n,4
    A["rotation"] = torch.stack([sum((qc[:, i].reshape(B, 1) * bh[..., _HAMILTON[k][i]]).abs() for i in range(4)) for k in range(4)], -1)
    rest = _flatten(net[:, 14:23]).reshape(B, HW, 3, 3)                                        # b n sh rgb
    v = torch.tensor(V_TO_SH, dtype=torch.float64)
    Tm = v.T @ M[:, :3, :3] @ v                                                                 # B,3(s),3(t)
    A["features_rest"] = torch.einsum("bnsc,bst->bntc", rest.abs(), Tm.abs())
    clamped = torch.zeros(B, HW, 3, dtype=torch.bool)
    fragile = torch.zeros(B, HW, 3, dtype=torch.bool)
    if squre_clip < 10.0:
        c = float(np.float32(squre_clip))                                                       # the value the kernel receives
        fragile[..., :2] = (X[..., :2].abs() - c).abs() <= 2.0 ** -18 * c
        clamped[..., :2] = (X[..., :2].abs() > c) & ~fragile[..., :2]
    return {"out": out, "A": A, "clamped": clamped, "fragile": fragile, "den": den, "clip": squre_clip}


def forward_K(got, tr, label=""):
    """``got``: {key: float32 tensor [B,n,...]} of an implementation. Returns ({group: 1-D K over the ordinary elements}, [messages of
    broken exactness / special-value rules])."""
    import forward_bars as FB
    ks, bad = {}, []
    for g in K_GROUPS:
        x, t, A = got[g].detach().cpu(), tr["out"][g], tr["A"][g]
        sel = torch.ones_like(t, dtype=torch.bool)
        if g == "xyz":
            sel = ~(tr["clamped"] | tr["fragile"])
            c = float(np.float32(tr["clip"]))
            want = torch.sign(t[tr["clamped"]]) * c
            if not torch.equal(x.double()[tr["clamped"]], want):
                bad.append(f"{label}: a clamped x / y is not +-float32(squre_clip) to the bit")
        bad += FB.special_failures(x, t, A, sel, f"{label} {g}")
        ks[g] = FB.k_of(x, t, A, sel)
    return ks, bad


def copies_bit_equal(got, inputs):
    """features_dc and unet_depth are the inputs' bits (compared as int32: NaN payloads and signed zeros included)."""
    net, depth = inputs["net_out"].detach().cpu().float(), inputs["depth"].detach().cpu().float()
    B = net.shape[0]
    bits = lambda t: t.contiguous().view(torch.int32)
    return (torch.equal(bits(got["features_dc"].detach().cpu()), bits(_flatten(net[:, 11:14]).unsqueeze(2).contiguous()))
            and torch.equal(bits(got["unet_depth"].detach().cpu()), bits(_flatten(depth.reshape(B, 1, -1)).contiguous())))


def _camera(gen, perspective=None):
    """A seeded view_to_world (row-vector convention: [p,1] @ M) and camera quaternion: a rotation of 0.3..1.3 rad, a translation of
    about 0.5; ``perspective`` = (column [3], m33) fills the fourth column."""
    axis = torch.randn(3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm()
    ang = 0.3 + float(torch.rand(1, generator=gen, dtype=torch.float64))
    Kx = torch.tensor([[0., -axis[2], axis[1]], [axis[2], 0., -axis[0]], [-axis[1], axis[0], 0.]], dtype=torch.float64)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(ang) * Kx + (1 - math.cos(ang)) * (Kx @ Kx)
    M[3, :3] = torch.randn(3, generator=gen, dtype=torch.float64) * 0.5
    if perspective is not None:
        M[:3, 3] = torch.tensor(perspective[0], dtype=torch.float64)
        M[3, 3] = perspective[1]
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    return M.float(), (q / q.norm()).float()


def seeded_inputs(B, H, W, seed, perspective=None):
    """Seeded inputs of any shape: offsets 0.5 noise, scaling logits around log 0.01, depth 1..3, seeded ``ray_dirs`` (x, y in +-0.3, z = 1),
    a camera and a quaternion of its own per image."""
    gen = torch.Generator().manual_seed(4200 + seed)
    net = torch.randn(B, 23, H, W, generator=gen) * 0.5
    net[:, 4:7] = net[:, 4:7] * 0.3 + math.log(0.01)
    cams = [_camera(gen, None if perspective is None else perspective[b]) for b in range(B)]
    return {"net_out": net.contiguous(), "depth": torch.rand(B, 1, H, W, generator=gen) * 2.0 + 1.0,
            "ray_dirs": torch.cat([torch.rand(1, 2, H, W, generator=gen) * 0.6 - 0.3, torch.ones(1, 1, H, W)], 1).contiguous(),
            "v2w": torch.stack([c[0] for c in cams]).contiguous(), "quat": torch.stack([c[1] for c in cams]).contiguous()}


def conj_pixels(H, W):
    """Flat pixel indices of the quaternion case: (exact conj(cam_quat), 0.7 conj(cam_quat) + 1e-6 (+-1, +-1, +-1, +-1))."""
    n = torch.arange(H * W)
    return n[n % 8 == 6], n[n % 8 == 7]


_CASES = None


def forward_cases():
    """{name: (inputs, squre_clip, pooled)}: built once, never modified. ``pooled``: an ordinary case, whose K enters the pooled bars;
    the saturation and quaternion cases are held case by case (max K) and by the special-value rules."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = {"fixture": (load_inputs()[0], 10000.0, True), "fixture_clip": (load_inputs()[0], 0.3, True),
             "35px": (seeded_inputs(3, 5, 7, 1), 10000.0, True),
             # a perspective fourth column: w3 = p . column + m33 lies in 0.5 .. 2, so the divide matters
             "289px_persp": (seeded_inputs(2, 17, 17, 2, perspective=(((0.02, -0.02, 0.15), 0.8), ((-0.02, 0.03, 0.18), 0.8))), 10000.0, True),
             "1px": (seeded_inputs(1, 1, 1, 3), 10000.0, True)}
    far = seeded_inputs(2, 17, 17, 4)                   # offsets that push some |X| beyond 10
    n = torch.arange(17 * 17).reshape(17, 17)
    far["net_out"][:, 0] += torch.where(n % 7 == 0, 25.0, 0.0) * torch.where(n % 2 == 0, 1.0, -1.0)
    far["net_out"][:, 1] += torch.where(n % 11 == 0, -30.0, 0.0)
    for clip in (0.3, 9.999, 10.0):
        cases[f"clip_{clip:g}"] = (far, clip, True)
    sat = seeded_inputs(2, 5, 7, 5)
    n = torch.arange(35).reshape(5, 7)
    for b in range(2):
        sat["net_out"][b, 3] = torch.tensor(OPACITY_LOGITS)[(n + b) % 8]
        for c in range(3):
            sat["net_out"][b, 4 + c] = torch.tensor(SCALING_LOGITS)[(n + b + c) % 6]
    cases["saturation"] = (sat, 10000.0, False)
    qt = seeded_inputs(2, 5, 7, 6)
    gen = torch.Generator().manual_seed(77)
    exact, near = conj_pixels(5, 7)
    for b in range(2):
        q = torch.randn(35, 4, generator=gen, dtype=torch.float64)              # negative components included
        q = q / q.norm(dim=1, keepdim=True) * torch.tensor(QUAT_NORMS, dtype=torch.float64)[torch.arange(35) % 8 % 6].unsqueeze(1)
        conj = qt["quat"][b].double() * torch.tensor([1., -1., -1., -1.], dtype=torch.float64)
        q[exact] = conj                                                          # three output components cancel exactly
        signs = torch.tensor([[1., -1., 1., -1.], [1., 1., -1., -1.], [-1., 1., 1., -1.], [1., -1., -1., 1.]], dtype=torch.float64)
        q[near] = conj * 0.7 + 1e-6 * signs[torch.arange(len(near)) % 4]        # ... and to about 1e-6: under a 3e-6 whole-tensor gate
        qt["net_out"][b, 7:11] = q.float().T.reshape(4, 5, 7)
    cases["quaternions"] = (qt, 10000.0, False)
    _CASES = cases
    return cases


_TRUTHS = {}


def case_truth(name):
    """(forward_truth, K of the float32 restatement, the restatement's float32 outputs) of a case: computed once."""
    if name not in _TRUTHS:
        inputs, clip, _ = forward_cases()[name]
        tr = forward_truth(inputs, clip)
        with torch.no_grad():
            r32 = splat_head_torch(inputs["net_out"], inputs["depth"], inputs["ray_dirs"], inputs["v2w"], inputs["quat"], clip)
        ks, bad = forward_K(r32, tr, f"restatement {name}")
        _TRUTHS[name] = (tr, ks, bad, r32)
    return _TRUTHS[name]
