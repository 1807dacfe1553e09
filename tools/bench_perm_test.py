#!/usr/bin/env python3
"""The permutation two-sample test at the ECPE test-set shape: n_1 = n_2 = 1 938 latents of width 24, P = 1 000 relabellings.
Timed with device events, each part warmed up and then run `--reps` times back to back inside one event pair (time per call = window /
reps); the torch formulations run on the same GPU on the same matrix and labels:
  * label generation (torch: rand, stable argsort, scatter),
  * carel_rbf_gram (one launch),
  * carel_mmd_perm_test (three launches),
  * the statistic in plain torch: q = ((G @ M') * G).sum(1), l = G @ (R + C), the three sums and the count, in float32 and in float64
    (float64 is the accuracy yardstick: the worst |stats - float64| as a fraction of the bound of tests/perm_restate.py is reported
    for the kernels and for torch float32),
  * one pair_latents call on n_1 ECPE-shaped pairs (12 layers), for scale.
Prints one JSON line.   python tools/bench_perm_test.py [--n 1938] [--d 24] [--perms 1000] [--reps 20] [--layers 12]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from carel_vae_amd import drl_classifier as M, data as D, ops
from tests import perm_restate as PR

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1938, help="rows per sample")
ap.add_argument("--d", type=int, default=24)
ap.add_argument("--perms", type=int, default=1000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--layers", type=int, default=12, help="encoder layers of the pair_latents call (0 = skip it)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_perm_test.py needs the GPU: nothing here is measured without one")

n1 = n2 = a.n
n, P = n1 + n2, a.perms
coef = PR.mmd_coefficients(n1, n2)
g = torch.Generator(device="cuda").manual_seed(1)
s1 = torch.randn((n1, a.d), device="cuda", generator=g)
s2 = torch.randn((n2, a.d), device="cuda", generator=g)
alphas = list(ops.MODEL_MMD_ALPHAS)


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def torch_stats(K, labels, dtype):
    """the issue's quadratic form on the device -> (stats, count)"""
    Mz = K.to(dtype).clone()
    Mz.fill_diagonal_(0)
    G = labels.to(dtype)
    q = ((G @ Mz) * G).sum(1)
    l = G @ (Mz.sum(1) + Mz.sum(0))
    S01 = l - 2 * q
    S00 = Mz.sum() - q - S01
    stats = coef[0] * S00 + coef[2] * q + coef[1] * S01
    return stats, (stats[1:] >= stats[0]).sum()


labels = M.random_labellings(n1, n2, P, "cuda", torch.Generator(device="cuda").manual_seed(2))
K = ops.rbf_gram(s1, s2, alphas)
t_labels = event_ms(lambda: M.random_labellings(n1, n2, P, "cuda", g), a.reps)
t_gram = event_ms(lambda: ops.rbf_gram(s1, s2, alphas), a.reps)
t_perm = event_ms(lambda: ops.mmd_perm_test(K, labels, n1, n2, *coef), a.reps)
t_t32 = event_ms(lambda: torch_stats(K, labels, torch.float32), a.reps)
t_t64 = event_ms(lambda: torch_stats(K, labels, torch.float64), max(a.reps // 4, 2))

stats, count = ops.mmd_perm_test(K, labels, n1, n2, *coef)
s64, c64 = torch_stats(K, labels, torch.float64)
s32, c32 = torch_stats(K, labels, torch.float32)
bound = torch.from_numpy(PR.stats_bound(K.cpu().numpy(), labels.cpu().numpy(), coef)).cuda()
frac_kernel = float(((stats - s64).abs() / bound).max())
frac_torch32 = float(((s32.double() - s64).abs() / bound).max())
undecided = int(((s64[1:] - s64[0]).abs() <= bound[1:] + bound[0]).sum())

t_lat = None
if a.layers > 0:
    cfg = M.encoder_config("zh", layers=a.layers)
    model = M.DrlClassifier(M.make_opt(pair_bow_dim=8), cfg, seed=1).to("cuda").eval()
    b = D.synthetic_ecpe_batch(n1, 128, cfg.vocab_size, 8, seed=9, shape="B")
    ids, att, tt = (b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
    t_lat = event_ms(lambda: model.pair_latents(ids, att, tt), max(a.reps // 4, 2))

flop = 4.0 * n * n * (P + 1)          # two 0 / 1 products of [n, n] x [n, P + 1]
print(json.dumps(dict(n1=n1, n2=n2, d=a.d, perms=P, reps=a.reps, labels_ms=round(t_labels, 4), gram_ms=round(t_gram, 4),
                      perm_test_ms=round(t_perm, 4), perm_test_tflops=round(flop / (t_perm * 1e-3) / 1e12, 2),
                      torch_f32_ms=round(t_t32, 4), torch_f64_ms=round(t_t64, 4),
                      pair_latents_ms=None if t_lat is None else round(t_lat, 3),
                      count=int(count), count_f64=int(c64), count_torch_f32=int(c32), undecided=undecided,
                      frac_of_bound_kernel=round(frac_kernel, 4), frac_of_bound_torch_f32=round(frac_torch32, 4),
                      mmd=float(stats[0]), pval=int(count) / P)), flush=True)
