#!/usr/bin/env python3
"""What opt.train_adapter costs per training step: the dense B = 64, S = 128, 12-layer step with the entmax adapters and FusedAdam, the
frozen-adapter model (the reference's behaviour) and the trained-adapter model interleaved step by step in ONE process (same clocks,
same neighbours); median of 20 steps after 5 warm-ups each, timed with events.  The difference should be one more read of the last
hidden states (25 MB), carel_adapter_backward_weights' five launches and Adam over 2.4 M (raw: 4.7 M) more elements.

    python tools/bench_adapter_train.py [--steps 20] [--warmup 5] [--adapter entmax]
    rocprofv3 --kernel-trace --stats -d out/adapter_trace -- python tools/bench_adapter_train.py      # per-kernel times (adapter_wgrad_*)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from carel_vae_amd import drl_classifier as M  # noqa: E402
from carel_vae_amd.data import synthetic_ecpe_batch  # noqa: E402

B, S, V = 64, 128, 23771


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--adapter", default="entmax", choices=["entmax", "sparsemax", "raw"])
    a = ap.parse_args()
    cfg = M.encoder_config("zh")
    batch = {k: v.cuda() for k, v in synthetic_ecpe_batch(B, S, cfg.vocab_size, V, seed=3, shape="A").items()}
    args = lambda i: (batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], batch["emo_labels"], batch["cau_labels"],   # noqa: E731
                      batch["labels"], batch["bow_reps"], i % 41)
    models = {}
    for name, kw in (("frozen", {}), ("trained", dict(train_adapter=True))):
        opt = M.make_opt(pair_bow_dim=V, adapter=a.adapter, **kw)
        m = M.DrlClassifier(opt, cfg, seed=0).to("cuda").train()
        models[name] = (m, M.FusedAdam(m, lr=1e-5, fuse_into_backward=True))

    def step(name, i):
        m, o = models[name]
        loss = m(*args(i))
        o.zero_grad()
        loss.backward()
        o.step()

    times = {k: [] for k in models}
    for i in range(a.warmup + a.steps):
        for name in models:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            step(name, i)
            t1.record()
            t1.synchronize()
            if i >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {k + "_ms_median": round(statistics.median(v), 4) for k, v in times.items()}
    res.update({k + "_ms_min": round(min(v), 4) for k, v in times.items()})
    res["delta_ms_median"] = round(res["trained_ms_median"] - res["frozen_ms_median"], 4)
    res["delta_percent"] = round(100.0 * res["delta_ms_median"] / res["frozen_ms_median"], 2)
    res.update(adapter=a.adapter, batch=B, seq_len=S, layers=cfg.layers, steps=a.steps, warmup=a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
