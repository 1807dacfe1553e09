#!/usr/bin/env python3
"""Re-evaluation with fresh noise (the case analysis' `while True`, mmd_wommd_case_analysis.py:662-696): N ECPE-shaped pairs, 12 layers.
Times (wall clock, device drained, results on the host each time)
  * one pair_latents call,
  * K draws through draw_counts on those latents (TP / FP / FN per draw read back),
  * K sequential get_pair_preds calls with the F1 computed on the host from each (the path without pair_latents),
  * K = 1 both ways: pair_latents + draw_counts(1) against one get_pair_preds + host F1.
Prints one JSON line.   python tools/bench_draws.py [--pairs 1938] [--draws 1000] [--sequential 1000] [--layers 12]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from carel_vae_amd import drl_classifier as M, data as D, training as T

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1938)
ap.add_argument("--draws", type=int, default=1000)
ap.add_argument("--sequential", type=int, default=1000, help="sequential get_pair_preds calls actually run (the time is reported per call and scaled to --draws)")
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

cfg = M.encoder_config("zh", layers=a.layers)
model = M.DrlClassifier(M.make_opt(pair_bow_dim=8), cfg, seed=1).to("cuda").eval()
b = D.synthetic_ecpe_batch(a.pairs, 128, cfg.vocab_size, 8, seed=9, shape="B")
ids, att, tt = (b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
labels = b["labels"].cuda()
host_labels = b["labels"].numpy().tolist()


def median_ms(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e3 * ts[len(ts) // 2]


def f1_of_counts(lat, k):
    return T.prf_from_counts(model.draw_counts(lat, labels, k).sum(1))[2].cpu()


def f1_sequential():
    return T._prf1(host_labels, model.get_pair_preds(ids, att, tt))[2]


lat = model.pair_latents(ids, att, tt)
t_lat = median_ms(lambda: model.pair_latents(ids, att, tt), a.reps)
t_draws = median_ms(lambda: f1_of_counts(lat, a.draws), a.reps)
t_new_k1 = median_ms(lambda: f1_of_counts(model.pair_latents(ids, att, tt), 1), a.reps)
t_seq_k1 = median_ms(f1_sequential, a.reps)
f1_sequential(); torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.sequential):
    f1_sequential()
torch.cuda.synchronize()
t_seq_call = 1e3 * (time.perf_counter() - t0) / max(a.sequential, 1)
t_seq = t_seq_call * a.draws
print(json.dumps(dict(pairs=a.pairs, layers=a.layers, draws=a.draws, sequential_calls_run=a.sequential, pair_latents_ms=round(t_lat, 3),
                      draw_counts_ms=round(t_draws, 3), sequential_ms=round(t_seq, 1), sequential_ms_per_call=round(t_seq_call, 3),
                      speedup=round(t_seq / (t_lat + t_draws), 1), k1_new_ms=round(t_new_k1, 3), k1_sequential_ms=round(t_seq_k1, 3))), flush=True)
