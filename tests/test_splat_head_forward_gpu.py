"""The splat head's forward kernel (f3dg_splat_head, f3d.splat_head, _SplatHead, splat_head_merge) against float64 on its own inputs,
element by element (truth, scales and cases: tests/splat_head_truth.py, proven on the host by
tests/test_splat_head_forward_truth.py).

    K = |x - truth| / (2^-24 A);  per group, pooled over the ordinary cases: the kernel's median, p99 and max of K each <= 4 x the float32
    restatement's on the same inputs; every case alone: max K <= 4 x the restatement's pooled max.

Every output starts as a NaN sentinel bit pattern, so a skipped element shows; every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import f3dgaus_amd as f3d
from f3dgaus_amd import _lib
from f3dgaus_amd.gaussian_predictor import _KEY_SHAPE, _SplatHead, allocate_gaussians
import forward_bars as FB
import splat_head_truth as T

pytestmark = pytest.mark.gpu
KEYS = T.KEYS
CASES = tuple(T.forward_cases())
POOLED = tuple(n for n in CASES if T.forward_cases()[n][2])
SENTINEL = 0x7FC0BEEF               # a quiet NaN with a payload: neither a result nor torch's default NaN


def _sentinel_buffers(B, n_total, dev):
    out = allocate_gaussians(B, n_total, dev)
    for k in KEYS:
        out[k].view(torch.int32).fill_(SENTINEL)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _raw(inputs, clip, dev, n_total=None, n_offset=0):
    """f3dg_splat_head through ctypes into sentinel-filled buffers [B, n_total, ...]; returns the buffers."""
    t = {k: v.to(dev).contiguous() for k, v in inputs.items()}
    B, _, H, W = t["net_out"].shape
    n_total = H * W if n_total is None else n_total
    assert 0 <= n_offset <= n_total - H * W
    out = _sentinel_buffers(B, n_total, dev)
    rc = _lib.lib().f3dg_splat_head(C.c_void_p(torch.cuda.current_stream().cuda_stream), B, H, W, _lib.ptr(t["net_out"]), _lib.ptr(t["depth"]),
                                    _lib.ptr(t["ray_dirs"]), _lib.ptr(t["v2w"]), _lib.ptr(t["quat"]), float(clip), n_total, n_offset,
                                    *[_lib.ptr(out[k]) for k in KEYS])
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return out


def _wrapper(inputs, clip, dev, **kw):
    t = {k: v.to(dev) for k, v in inputs.items()}
    with torch.no_grad():
        return f3d.splat_head(t["net_out"], t["depth"], t["ray_dirs"], t["v2w"], t["quat"], squre_clip=clip, **kw)


def test_every_element_against_float64(gpu_device):
    """All cases through the raw entry point: the bars per group, the exactness rules (copies, clamped x / y) and the special values."""
    k_ker, k_ref, bad = {}, {}, []
    for name in CASES:
        inputs, clip, _ = T.forward_cases()[name]
        tr, ks_ref, bad_ref, _ = T.case_truth(name)
        assert not bad_ref, bad_ref
        out = {k: v.cpu() for k, v in _raw(inputs, clip, gpu_device).items()}
        for k in KEYS:
            assert not bool((_bits(out[k]) == SENTINEL).any()), (name, k, "an element was not written")
            assert tuple(out[k].shape[2:]) == _KEY_SHAPE[k]
        if not T.copies_bit_equal(out, inputs):
            bad.append(f"{name}: features_dc / unet_depth are not the inputs' bits")
        k_ker[name], b = T.forward_K(out, tr, name)
        k_ref[name] = ks_ref
        bad += b
    broken = FB.hold_to_bars(k_ker, k_ref, POOLED, "splat head")
    print("rules:", bad, "\nbars:", broken)
    assert not bad and not broken, (bad, broken)


def test_clip_thresholds(gpu_device):
    """squre_clip 10.0 takes the `< 10` switch's other side: bit-identical to no clip at all, with |X| beyond 10 present; at 9.999 exactly
    those are clamped, to float32(9.999); at 0.3 every other group is bit-identical to the unclipped run."""
    inputs = T.forward_cases()["clip_10"][0]
    free = _raw(inputs, 10000.0, gpu_device)
    at10, at9, at03 = (_raw(inputs, c, gpu_device) for c in (10.0, 9.999, 0.3))
    for k in KEYS:
        assert torch.equal(_bits(at10[k]), _bits(free[k])), k
        if k != "xyz":
            assert torch.equal(_bits(at9[k]), _bits(free[k])) and torch.equal(_bits(at03[k]), _bits(free[k])), k
    xy = free["xyz"][..., :2]
    beyond = xy.abs() > 10.0
    print("clip: |X| > 10:", int(beyond.sum()), " |X| > 0.3:", int((xy.abs() > 0.3).sum()), "of", xy.numel())
    assert int(beyond.sum()) > 20
    c9 = torch.tensor(9.999, dtype=torch.float32, device=gpu_device)
    assert torch.equal(at9["xyz"][..., :2], torch.where(beyond, torch.sign(xy) * c9, xy))
    assert torch.equal(at9["xyz"][..., 2], free["xyz"][..., 2]) and torch.equal(at03["xyz"][..., 2], free["xyz"][..., 2])


def test_non_finite_inputs_stay_in_their_own_outputs(gpu_device):
    """One NaN / +Inf / -Inf in each input channel in turn (23 of net_out, then depth), at one pixel of one image: only the outputs that
    depend on that channel at that pixel may change; every other element of every output is bit-identical to the clean run. A NaN
    does arrive in each of them; under a clip a NaN position stays NaN as torch.clamp leaves it."""
    inputs = T.forward_cases()["35px"][0]
    B, _, H, W = inputs["net_out"].shape
    clean = {k: _bits(v) for k, v in _raw(inputs, 10000.0, gpu_device).items()}
    b, n = 1, 17
    y, x = divmod(n, W)
    values = (float("nan"), float("inf"), -float("inf"))

    def dependents(ch):
        """{key: bool mask over the trailing dims} of the outputs that read input channel ``ch`` (23: depth)."""
        m = {}
        if ch < 3 or ch == 23:
            m["xyz"] = torch.ones(3, dtype=torch.bool)
        if ch == 23:
            m["unet_depth"] = torch.ones(1, dtype=torch.bool)
        if ch == 3:
            m["opacity"] = torch.ones(1, dtype=torch.bool)
        if 4 <= ch < 7:
            m["scaling"] = torch.arange(3) == ch - 4
        if 7 <= ch < 11:
            m["rotation"] = torch.ones(4, dtype=torch.bool)
        if 11 <= ch < 14:
            m["features_dc"] = (torch.arange(3) == ch - 11).reshape(1, 3)
        if 14 <= ch < 23:
            m["features_rest"] = (torch.arange(3) == (ch - 14) % 3).reshape(1, 3).expand(3, 3)      # [t][c]: all three t of colour c
        return m

    for ch in range(24):
        for val in (values[ch % 3], values[0]):
            poisoned = {k: v.clone() for k, v in inputs.items()}
            if ch < 23:
                poisoned["net_out"][b, ch, y, x] = val
            else:
                poisoned["depth"][b, 0, y, x] = val
            got = _raw(poisoned, 10000.0, gpu_device)
            dep = dependents(ch)
            for k in KEYS:
                may = torch.zeros(clean[k].shape, dtype=torch.bool)
                if k in dep:
                    may[b, n] = dep[k]
                same = _bits(got[k]).cpu() == clean[k].cpu()
                assert bool(same[~may].all()), (ch, val, k, "a non-finite input reached an output that does not depend on it")
                if k in dep and val != val:
                    assert bool(torch.isnan(got[k].cpu()[may]).all()), (ch, k, "a NaN input did not arrive")
    poisoned = {k: v.clone() for k, v in inputs.items()}
    poisoned["net_out"][b, 0, y, x] = float("nan")
    clipped, clean_clip = _raw(poisoned, 0.3, gpu_device), _raw(inputs, 0.3, gpu_device)
    assert bool(torch.isnan(clipped["xyz"][b, n]).all())
    keep = torch.ones(B, H * W, dtype=torch.bool)
    keep[b, n] = False
    assert torch.equal(_bits(clipped["xyz"]).cpu()[keep], _bits(clean_clip["xyz"]).cpu()[keep])


def test_merged_buffers_and_the_other_forms(gpu_device):
    """Rows outside n_offset .. n_offset + HW of a K = 3 merged buffer keep their sentinel bits, for each of the three windows; the
    out= form, the autograd form (_SplatHead) and splat_head_merge are bit-identical to the plain form."""
    dev = gpu_device
    inputs = T.forward_cases()["289px_persp"][0]
    B, _, H, W = inputs["net_out"].shape
    HW = H * W
    plain = _wrapper(inputs, 0.3, dev)
    raw = _raw(inputs, 0.3, dev)
    for k in KEYS:
        assert torch.equal(_bits(plain[k]), _bits(raw[k])), k
    for slot in range(3):
        for form in ("raw", "out="):
            if form == "raw":
                merged = _raw(inputs, 0.3, dev, n_total=3 * HW, n_offset=slot * HW)
            else:
                merged = _sentinel_buffers(B, 3 * HW, dev)
                assert _wrapper(inputs, 0.3, dev, out=merged, n_offset=slot * HW) is merged
            for k in KEYS:
                bits = _bits(merged[k])
                assert torch.equal(bits[:, slot * HW:(slot + 1) * HW], _bits(plain[k])), (form, slot, k)
                outside = torch.cat([bits[:, :slot * HW], bits[:, (slot + 1) * HW:]], 1)
                assert bool((outside == SENTINEL).all()), (form, slot, k, "a row outside the window was written")
    t = {k: v.to(dev) for k, v in inputs.items()}
    graph = f3d.splat_head(t["net_out"].clone().requires_grad_(), t["depth"], t["ray_dirs"], t["v2w"], t["quat"], squre_clip=0.3)
    direct = _SplatHead.apply(t["net_out"].contiguous(), t["depth"].contiguous(), t["ray_dirs"].contiguous(), t["v2w"].reshape(B, 16).contiguous(),
                              t["quat"].contiguous(), 0.3)
    for i, k in enumerate(KEYS):
        assert graph[k].grad_fn is not None
        assert torch.equal(_bits(graph[k].detach()), _bits(plain[k])) and torch.equal(_bits(direct[i]), _bits(plain[k])), k
    # three passes (the second with other cameras) merged: without and with autograd
    second = dict(inputs, v2w=inputs["v2w"].flip(0).contiguous(), quat=inputs["quat"].flip(0).contiguous())
    passes = [inputs, second, inputs]
    singles = [_wrapper(p, 0.3, dev) for p in passes]
    to = lambda key: [p[key].to(dev) for p in passes]
    with torch.no_grad():
        m0 = f3d.splat_head_merge(to("net_out"), to("depth"), t["ray_dirs"], to("v2w"), to("quat"), squre_clip=0.3)
    nets = [n.requires_grad_() for n in to("net_out")]
    m1 = f3d.splat_head_merge(nets, to("depth"), t["ray_dirs"], to("v2w"), to("quat"), squre_clip=0.3)
    for k in KEYS:
        want = torch.cat([s[k] for s in singles], 1)
        assert m1[k].grad_fn is not None and m0[k].grad_fn is None
        assert torch.equal(_bits(m0[k]), _bits(want)) and torch.equal(_bits(m1[k].detach()), _bits(want)), k
    assert not torch.equal(singles[0]["xyz"], singles[1]["xyz"])


def test_two_runs_are_bit_identical(gpu_device):
    for name in ("fixture_clip", "quaternions", "saturation"):
        inputs, clip, _ = T.forward_cases()[name]
        a, b = _raw(inputs, clip, gpu_device), _raw(inputs, clip, gpu_device)
        for k in KEYS:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (name, k)


def test_wrong_shapes_are_refused_on_the_device_and_a_valid_call_follows(gpu_device):
    """The wrappers raise before any launch (the checks themselves: tests/test_splat_head_forward_truth.py); a valid call right after
    gives the plain result."""
    dev = gpu_device
    inputs = T.forward_cases()["35px"][0]
    t = {k: v.to(dev) for k, v in inputs.items()}
    B, _, H, W = t["net_out"].shape
    HW = H * W
    args = lambda **kw: (kw.get("net_out", t["net_out"]), kw.get("depth", t["depth"]), kw.get("ray_dirs", t["ray_dirs"]), t["v2w"], t["quat"])
    ok = allocate_gaussians(B, 2 * HW, dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="depth"):
            f3d.splat_head(*args(depth=t["depth"][:, :, :-1]))
        with pytest.raises(ValueError, match="ray_dirs"):
            f3d.splat_head(*args(ray_dirs=t["ray_dirs"][:, :, :, :-1]))
        with pytest.raises(ValueError, match="xyz"):
            f3d.splat_head(*args(), out={**ok, "xyz": torch.zeros(B, 2 * HW, 1, device=dev)})
        with pytest.raises(ValueError, match="n_offset"):
            f3d.splat_head(*args(), out=ok, n_offset=HW + 1)
        with pytest.raises(RuntimeError, match="is on"):
            f3d.splat_head(*args(), out={**ok, "opacity": torch.zeros(B, 2 * HW, 1)})
        with pytest.raises(ValueError, match="pass 1: depth"):
            f3d.splat_head_merge([t["net_out"]] * 2, [t["depth"], t["depth"][:, :, :-1]], t["ray_dirs"], [t["v2w"]] * 2, [t["quat"]] * 2)
        got = f3d.splat_head(*args(), out=ok, n_offset=HW)
    plain = _raw(inputs, 10000.0, dev)
    for k in KEYS:
        assert torch.equal(_bits(got[k][:, HW:]), _bits(plain[k])), k
