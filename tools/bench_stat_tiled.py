#!/usr/bin/env python3
"""The tiled differentiable statistics (carel_hsic_tiled_fwd/bwd, carel_rbf_mmd_tiled_fwd/bwd), forward + backward, at
  HSIC  m = 757 (the single-workgroup operator's top size at d = 24), 1 938 (the ECPE test set's pairs), 8 192 (the row limit);
  MMD   n1 = n2 = 786 (the single-workgroup top size), 1 938, 4 096 (the row limit), with one and with three alphas;   d = 24,
against, on the same GPU and the same samples,
  * the single-workgroup operator (carel_hsic_fwd/bwd, carel_rbf_mmd_fwd/bwd) at its top size,
  * torch float32 autograd of the matrix form (tests/stats_restate.py: hsic_formula / mmd_formula, on the device),
  * the same in float64 (also the yardstick of the printed differences).
Timed with device events.  Every part is warmed up; then the parts of a shape are run INTERLEAVED, one window of `reps` back-to-back
calls each per round, for `--windows` rounds; the median window (time per call = window / reps) is reported with the range, so that a
disturbance from other work on the machine hits every part alike.  Prints one JSON line per shape.
    python tools/bench_stat_tiled.py [--d 24] [--reps 3] [--windows 5] [--no-f64-above 8192]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from carel_vae_amd import ops
from tests import stats_restate as R

ap = argparse.ArgumentParser()
ap.add_argument("--d", type=int, default=24)
ap.add_argument("--reps", type=int, default=3, help="calls per window of the kernels (torch: one)")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--no-f64-above", type=int, default=8192, help="skip the torch float64 part above this many rows")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_stat_tiled.py needs the GPU: nothing here is measured without one")
d = a.d
gen = torch.Generator(device="cuda").manual_seed(1)
one = torch.ones(1, device="cuda")


def hsic_matrix_form(x, y, s_x, s_y):
    """stats_restate.hsic_formula with H built on the samples' device"""
    m = x.shape[0]
    K, L = torch.exp(-R._pairwise(x) / s_x), torch.exp(-R._pairwise(y) / s_y)
    H = torch.eye(m, dtype=x.dtype, device=x.device) - 1.0 / m
    return torch.trace(L @ (H @ (K @ H))) / ((m - 1) ** 2)


def autograd(form, dtype, *samples):
    leaves = [s.detach().to(dtype).requires_grad_(True) for s in samples]
    v = form(*leaves)
    v.backward()
    return (v.detach(),) + tuple(t.grad for t in leaves)


def window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def measure(tag, shape, parts, results):
    for fn, _ in parts.values():           # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in parts}
    for _ in range(a.windows):
        for k, (fn, reps) in parts.items():
            times[k].append(window_ms(fn, reps))
    out = dict(op=tag, d=d, reps=a.reps, windows=a.windows, **shape)
    for k, v in times.items():
        out[k + "_ms"] = round(statistics.median(v), 4)
        out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    res = {k: fn() for k, fn in results.items()}
    if "torch_f64" in res:
        ref = res["torch_f64"]
        for k, got in res.items():
            if k != "torch_f64":
                out[k + "_value_rel_diff"] = float((got[0].double() - ref[0]).abs() / ref[0].abs())
                out[k + "_grad_max_diff_over_max"] = max(float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(got[1:], ref[1:]))
    print(json.dumps(out), flush=True)


for m in (757, 1938, 8192):
    x = 0.15 * torch.randn((m, d), device="cuda", generator=gen)
    y = 0.8 * x + 0.09 * torch.randn((m, d), device="cuda", generator=gen)
    tiled = lambda: (ops.hsic_tiled(x, y),) + ops.hsic_tiled_backward(x, y, one)
    parts = {"tiled": (tiled, a.reps)}
    results = {"tiled": tiled}
    if m <= ops.hsic_single_limit(d):
        single = lambda: (ops.hsic(x, y),) + ops.hsic_backward(x, y, one)
        parts["single_workgroup"] = (single, a.reps)
        results["single_workgroup"] = single
    f32 = lambda: autograd(lambda p, q: hsic_matrix_form(p, q, 1.0, 1.0), torch.float32, x, y)
    parts["torch_f32"] = (f32, 1)
    results["torch_f32"] = f32
    if m <= a.no_f64_above:
        f64 = lambda: autograd(lambda p, q: hsic_matrix_form(p, q, 1.0, 1.0), torch.float64, x, y)
        parts["torch_f64"] = (f64, 1)
        results["torch_f64"] = f64
    measure("hsic", dict(m=m), parts, results)

for n in (786, 1938, 4096):
    s1 = torch.randn((n, d), device="cuda", generator=gen)
    s2 = 1.2 * torch.randn((n, d), device="cuda", generator=gen) + 0.5
    scale = (12.0 / (2.0 * float(torch.cdist(torch.cat((s1, s2)).double(), torch.cat((s1, s2)).double()).max()) ** 2)) ** 0.5
    s1, s2 = s1 * scale, s2 * scale        # the largest exp argument: 12 with three alphas (the largest is 2.0), 0.6 with alpha = 0.1
    for alphas in (R.A1, R.A3):
        al = list(alphas)
        tiled = lambda: (ops.rbf_mmd_tiled(s1, s2, al),) + ops.rbf_mmd_tiled_backward(s1, s2, al, one)
        parts = {"tiled": (tiled, a.reps)}
        results = {"tiled": tiled}
        if 2 * n <= ops.mmd_single_limit(d):
            single = lambda: (ops.rbf_mmd(s1, s2, al)[0],) + ops.rbf_mmd_backward(s1, s2, al, one)
            parts["single_workgroup"] = (single, a.reps)
            results["single_workgroup"] = single
        f32 = lambda: autograd(lambda p, q: R.mmd_formula(p, q, R.f32_scalars(al), R.f32_scalars([1e-5])[0]), torch.float32, s1, s2)
        parts["torch_f32"] = (f32, 1)
        results["torch_f32"] = f32
        if 2 * n <= a.no_f64_above:
            f64 = lambda: autograd(lambda p, q: R.mmd_formula(p, q, R.f32_scalars(al), R.f32_scalars([1e-5])[0]), torch.float64, s1, s2)
            parts["torch_f64"] = (f64, 1)
            results["torch_f64"] = f64
        measure("mmd", dict(n1=n, n2=n, alphas=len(al)), parts, results)
