"""The figure and the bars of the forward-against-float64 tests of the splat head and the epilogue -- TEST INFRASTRUCTURE ONLY
(tests/splat_head_truth.py, tests/epilogue_truth.py and the four test files on them).

    K = |x - truth| / (2^-24 * A)          A: the element's error scale, evaluated in float64

Bars, per output group (4 is the project's margin for a float32 kernel against the float32 reference):
    pooled over the ordinary cases: median, p99 and max of K each <= 4 x the same statistic of the float32 restatement
    every case alone:               max K <= 4 x the restatement's pooled max
The yardstick is always the restatement's K on the same inputs, never the implementation under test."""
import numpy as np
import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126                               # the smallest normal float32: below it the hardware may flush to zero
F32_MAX = float(np.finfo(np.float32).max)
MARGIN = 4.0
FRAGILE_CAP = 0.005                              # a condition on the cases, not a measurement


def k_stats(k):
    """(median, p99, max) of a 1-D float64 tensor of K; an empty one gives zeros."""
    if k.numel() == 0:
        return (0.0, 0.0, 0.0)
    k = k.double().flatten()
    return (float(k.median()), float(torch.quantile(k, 0.99)), float(k.max()))


def fmt(s):
    return f"{s[0]:.2f} / {s[1]:.2f} / {s[2]:.2f}"


def special_failures(got, truth, scale, sel, label):
    """The special-value rules on the elements ``sel`` (bool): where the scale is below 2^-126 the result lies in [0, 2^-126] with the
    truth's sign (exactly 0 where the scale is 0); where |truth| exceeds the float32 maximum it is +-inf. Returns a list of messages."""
    bad = []
    g = got.double()
    small = sel & (scale < TINY)
    if bool(small.any()):
        gs, ts = g[small], truth[small]
        ok = (gs.abs() <= TINY) & ((gs == 0) | (torch.sign(gs) == torch.sign(ts)))
        if not bool(ok.all()):
            bad.append(f"{label}: {int((~ok).sum())} of {int(small.sum())} results under 2^-126 outside [0, 2^-126] or of the wrong sign")
    big = sel & (truth.abs() > F32_MAX)
    if bool(big.any()):
        ok = torch.isinf(g[big]) & (torch.sign(g[big]) == torch.sign(truth[big]))
        if not bool(ok.all()):
            bad.append(f"{label}: {int((~ok).sum())} of {int(big.sum())} overflowing results are not +-inf")
    return bad


def ordinary(truth, scale, sel):
    """The elements of ``sel`` held by K: scale at least 2^-126, |truth| within the float32 range."""
    return sel & (scale >= TINY) & (truth.abs() <= F32_MAX)


def k_of(got, truth, scale, sel):
    """K on the ordinary elements of ``sel``, as a 1-D float64 tensor (a non-finite result gives inf)."""
    m = ordinary(truth, scale, sel)
    k = (got.double()[m] - truth[m]).abs() / (U24 * scale[m])
    return torch.where(torch.isfinite(k), k, torch.full_like(k, float("inf")))


def hold_to_bars(k_impl, k_ref, pooled_cases, label, margin=MARGIN):
    """``k_impl`` / ``k_ref``: {case: {group: 1-D K}} of the implementation under test and of the float32 restatement on the same inputs.
    Prints every figure, then returns the list of broken bars (empty: all hold)."""
    groups = list(next(iter(k_ref.values())).keys())
    bad = []
    for g in groups:
        ref = k_stats(torch.cat([k_ref[c][g] for c in pooled_cases]))
        imp = k_stats(torch.cat([k_impl[c][g] for c in pooled_cases]))
        print(f"{label} {g:13s} pooled   restatement {fmt(ref)}   under test {fmt(imp)}   (K median / p99 / max)")
        for name, a, b in zip(("median", "p99", "max"), imp, ref):
            if not a <= margin * b:
                bad.append(f"{g} pooled {name}: {a:.3f} > {margin:g} x {b:.3f}")
        for c in k_impl:
            s, r = k_stats(k_impl[c][g]), k_stats(k_ref[c][g])
            print(f"{label} {g:13s} {c:14s} restatement {fmt(r)}   under test {fmt(s)}   n {k_impl[c][g].numel()}")
            if not s[2] <= margin * ref[2]:
                bad.append(f"{g} case {c} max: {s[2]:.3f} > {margin:g} x {ref[2]:.3f}")
    return bad
