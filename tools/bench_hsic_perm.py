#!/usr/bin/env python3
"""The permutation independence test at the ECPE test-set shape: m = 1 938 paired latents of width 24, P = 1 000 re-pairings.
Timed with device events.  Every part is warmed up; then the parts are run INTERLEAVED, one window of `reps` back-to-back calls each
per round, for `--windows` rounds, and the median window (time per call = window / reps) is reported, so that a disturbance from
other work on the machine hits every part alike.  The torch formulations run on the same GPU on the same matrices and permutations:
  * the permutations (torch: rand, stable argsort),
  * the two carel_hsic_gram launches,
  * carel_hsic_perm_test (eight launches),
  * the same statistic as a torch loop over the permutations, (Kc * L[p][:, p]).sum() with Kc = H K H formed once, in float32 and in
    float64 (float64 is the accuracy yardstick: the worst |stats - float64| as a fraction of the bound of tests/hsic_perm_restate.py
    is reported for the kernels and for torch float32 side by side),
  * one pair_latents call on m ECPE-shaped pairs (12 layers), for scale.
Prints one JSON line.   python tools/bench_hsic_perm.py [--m 1938] [--d 24] [--perms 1000] [--reps 5] [--windows 5] [--layers 12]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from carel_vae_amd import drl_classifier as M, data as D, ops
from tests import hsic_perm_restate as HR

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=1938, help="paired rows")
ap.add_argument("--d", type=int, default=24)
ap.add_argument("--perms", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5, help="calls per window of the kernels (the torch loops: one)")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--layers", type=int, default=12, help="encoder layers of the pair_latents call (0 = skip it)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_hsic_perm.py needs the GPU: nothing here is measured without one")

m, P = a.m, a.perms
g = torch.Generator(device="cuda").manual_seed(1)
x = 0.3 * torch.randn((m, a.d), device="cuda", generator=g)
y = 0.15 * x + 0.3 * torch.randn((m, a.d), device="cuda", generator=g)
perms = M.random_permutations(m, P, "cuda", torch.Generator(device="cuda").manual_seed(2))
K, Lm = ops.hsic_gram(x, 1.0), ops.hsic_gram(y, 1.0)


def centred(Kd):
    return Kd - Kd.sum(1, keepdim=True) / m - Kd.sum(0, keepdim=True) / m + Kd.sum() / (m * m)


def torch_stats(dtype, magnitude=False):
    """the loop the issue names -> (stats [P+1], count), and with magnitude the sum of |Kc| |L[p][:, p]| the bound is made of"""
    Kc, Ld = centred(K.to(dtype)), Lm.to(dtype)
    out, mag = torch.empty(P + 1, device="cuda", dtype=dtype), torch.empty(P + 1, device="cuda", dtype=dtype)
    idx = perms.long()
    for p in range(P + 1):
        Lp = Ld[idx[p]][:, idx[p]]
        out[p] = (Kc * Lp).sum()
        if magnitude:
            mag[p] = (Kc.abs() * Lp.abs()).sum()
    den = (m - 1.0) ** 2
    return out / den, (out[1:] >= out[0]).sum(), mag / den


parts = {
    "permutations": (lambda: M.random_permutations(m, P, "cuda", g), a.reps),
    "gram_x2": (lambda: (ops.hsic_gram(x, 1.0), ops.hsic_gram(y, 1.0)), a.reps),
    "perm_test": (lambda: ops.hsic_perm_test(K, Lm, perms), a.reps),
    "torch_f32": (lambda: torch_stats(torch.float32), 1),
    "torch_f64": (lambda: torch_stats(torch.float64), 1),
}
if a.layers > 0:
    cfg = M.encoder_config("zh", layers=a.layers)
    model = M.DrlClassifier(M.make_opt(pair_bow_dim=8), cfg, seed=1).to("cuda").eval()
    b = D.synthetic_ecpe_batch(m, 128, cfg.vocab_size, 8, seed=9, shape="B")
    ids, att, tt = (b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
    parts["pair_latents"] = (lambda: model.pair_latents(ids, att, tt), 1)


def window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


for fn, _ in parts.values():           # warm-up: code objects, the allocator's blocks
    fn()
    fn()
torch.cuda.synchronize()
times = {k: [] for k in parts}
for _ in range(a.windows):
    for k, (fn, reps) in parts.items():
        times[k].append(window_ms(fn, reps))
med = {k: statistics.median(v) for k, v in times.items()}

stats, count = ops.hsic_perm_test(K, Lm, perms)
s64, c64, mag = torch_stats(torch.float64, magnitude=True)
s32, c32, _ = torch_stats(torch.float32)
bound = HR.FACTOR * HR.U * mag
frac_kernel = float(((stats - s64).abs() / bound).max())
frac_torch32 = float(((s32.double() - s64).abs() / bound).max())
undecided = int(((s64[1:] - s64[0]).abs() <= bound[1:] + bound[0]).sum())

out = dict(m=m, d=a.d, perms=P, reps=a.reps, windows=a.windows)
for k, v in med.items():
    out[k + "_ms"] = round(v, 4)
    out[k + "_ms_min_max"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
out.update(gathered_fma_per_s=round((P + 1) * m * m / (med["perm_test"] * 1e-3), 0), count=int(count), count_f64=int(c64), count_torch_f32=int(c32),
           undecided=undecided, frac_of_bound_kernel=round(frac_kernel, 4), frac_of_bound_torch_f32=round(frac_torch32, 4),
           hsic=float(stats[0]), pval=int(count) / P)
print(json.dumps(out), flush=True)
