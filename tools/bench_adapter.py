"""Training-step time with and without the EMNLP sentence adapters (drl_classifier_ec_mmd_final_mul_emnlp.py --adapter).

    python tools/bench_adapter.py [--modes false,raw,sparsemax,entmax] [--shapes A,B] [--steps 20] [--warmup 5]

BERT-base geometry (12 layers), batch 64, S = 128, fused Adam; shape A = dense batch, shape B = ECPE-shaped lengths (~77 % padding).
Per mode and shape: the median of per-step event times over synchronised, warm steps (forward, backward, Adam).  Adapter mode always
runs the dense encoder (every position of the last layer is attended), so on shape B it pays the dense step: the number a token-packed
adapter path would be measured against.  One JSON line per (mode, shape).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carel_vae_amd import drl_classifier as M  # noqa: E402
from oracle import carel_oracle as O  # noqa: E402


def run(mode, shape, steps, warmup, batch, heads):
    cfg = O.EncoderConfig()
    model = M.DrlClassifier(M.make_opt(adapter=mode, head_number=heads), M.encoder_config("zh"), seed=0).to("cuda").train()
    optim = M.FusedAdam(model, lr=1e-5, fuse_into_backward=True)
    batches = []
    for i in range(4):
        b = O.synthetic_batch(batch, 128, cfg, model.opt.pair_bow_dim, seed=1 + i, shape=shape)
        batches.append({k: v.cuda() for k, v in b.items()})
    keys = ("input_ids", "attention_masks", "token_type_ids", "emo_labels", "cau_labels", "labels", "bow_reps")

    def step(i):
        b = batches[i % len(batches)]
        loss = model(*(b[k] for k in keys), i % 41)
        optim.zero_grad()
        loss.backward()
        optim.step()

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        step(warmup + i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    t = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
    tokens = sum(int(b["attention_masks"].sum()) for b in batches) / len(batches)
    return dict(mode=mode, head_number=heads if mode == "raw" else None, shape=shape, batch=batch, seq_len=128,
                attended_tokens_per_batch=tokens, median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1], steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="false,raw,sparsemax,entmax")
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--head-number", type=int, default=4)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        for mode in a.modes.split(","):
            print(json.dumps(run(mode, shape, a.steps, a.warmup, a.batch, a.head_number)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
