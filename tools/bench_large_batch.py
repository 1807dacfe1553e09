#!/usr/bin/env python3
"""What batches beyond the single-workgroup limit of carel_tail_losses buy: the 12-layer training step (S = 128, V = 23 771, dropout
0.1, FusedAdam) at B = 64, 128 and 256, dense and ECPE-shaped (packed), and the three tail calls (latents, losses, backward) alone at
B = 64 on the single-workgroup path, B = 64 forced through the batch-tiled entry, and B = 128, 256 and 1024 on the tiled path.
Protocol of tools/bench_adapter_train.py: ONE process, the configurations interleaved step by step (same clocks, same neighbours),
median of 20 after 5 warm-ups each, timed with events.

    python tools/bench_large_batch.py [--steps 20] [--warmup 5] [--batches 64,128,256] [--tail-batches 128,256,1024]
    rocprofv3 --kernel-trace --stats -d out/large_batch_trace -- python tools/bench_large_batch.py --batches 128 --tail-batches 128

Prints one JSON line: step_ms / pairs_per_s per (shape, B), their ratios to B = 64, tail_us per configuration and call, and
tail_ratio_256_over_64 = tiled tail at B = 256 over the single-workgroup tail at B = 64 (linear in B would be 4).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from carel_vae_amd import drl_classifier as M  # noqa: E402
from carel_vae_amd import ops  # noqa: E402
from carel_vae_amd.data import synthetic_ecpe_batch  # noqa: E402

S, V = 128, 23771


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def bench_steps(model, optim, cfg, batches, steps, warmup):
    data = {}
    for shape in ("A", "B"):
        for B in batches:
            data[(shape, B)] = {k: v.cuda() for k, v in synthetic_ecpe_batch(B, S, cfg.vocab_size, V, seed=3, shape=shape).items()}

    def step(key, i):
        b = data[key]
        loss = model(b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], i % 41)
        optim.zero_grad()
        loss.backward()
        optim.step()

    times = {k: [] for k in data}
    for i in range(warmup + steps):
        for key in data:
            torch.cuda.synchronize()
            ms = timed(lambda: step(key, i))
            if i >= warmup:
                times[key].append(ms)
    res = {}
    for (shape, B), v in times.items():
        name = ("dense" if shape == "A" else "ecpe") + "_b%d" % B
        med = statistics.median(v)
        res[name] = dict(step_ms_median=round(med, 4), step_ms_min=round(min(v), 4), pairs_per_s=round(1000.0 * B / med, 1))
    for shape in ("dense", "ecpe"):
        base = res.get("%s_b64" % shape)
        for B in batches:
            if base and B != 64:
                res["%s_pairs_per_s_b%d_over_b64" % (shape, B)] = round(res["%s_b%d" % (shape, B)]["pairs_per_s"] / base["pairs_per_s"], 4)
    return res


def bench_tail(model, tail_batches, steps, warmup):
    """latents / losses / backward by events.  Weights and gradient destinations are the model's own tail tensors."""
    W, G = model._tail_weights()
    opt, dev = model.opt, "cuda"
    limit = ops.tail_batch_limit(opt.ec_dim, opt.e_num_class)
    g = torch.Generator().manual_seed(5)
    cfgs = {}
    for name, B, tiled in [("b64_single", 64, False), ("b64_tiled", 64, True)] + [("b%d_tiled" % B, B, True) for B in tail_batches]:
        assert tiled or B <= limit
        buf = ops.TailBuffers(B, 1, opt.ec_dim, opt.e_num_class, V, dev)
        x = torch.randn((B, 768), generator=g).to(dev)
        labels = dict(emo=torch.randint(0, opt.e_num_class, (B,), generator=g).to(dev), cau=(torch.rand(B, generator=g) < 0.3).float().to(dev),
                      pair=(torch.rand(B, generator=g) < 0.3).float().to(dev), bow=(torch.rand((B, V), generator=g) < 1e-3).float().to(dev))
        labels["pair"][0] = 1.0
        eps = torch.randn(opt.ec_dim, generator=g).to(dev), torch.randn(opt.ec_dim, generator=g).to(dev)
        a = ops.tail_args(buf, x, W, labels, eps[0], eps[1], opt, 1.0, grads=G, drop=(opt.dropout, 7, 0))
        a._keep = (buf, x, labels, eps)
        cfgs[name] = (a, ops.tail_losses_tiled if tiled else ops.tail_losses)
    times = {k: dict(latents=[], losses=[], backward=[]) for k in cfgs}
    for i in range(warmup + steps):
        for name, (a, losses) in cfgs.items():
            torch.cuda.synchronize()
            t = dict(latents=timed(lambda: ops.tail_latents(a)), losses=timed(lambda: losses(a)), backward=timed(lambda: ops.tail_backward(a)))
            if i >= warmup:
                for k, v in t.items():
                    times[name][k].append(v)
    res = {}
    for name, t in times.items():
        res[name] = {k + "_us": round(1000.0 * statistics.median(v), 2) for k, v in t.items()}
        res[name]["total_us"] = round(sum(res[name].values()), 2)
    if "b256_tiled" in res:
        res["tail_ratio_256_over_64"] = round(res["b256_tiled"]["total_us"] / res["b64_single"]["total_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="64,128,256")
    ap.add_argument("--tail-batches", default="128,256,1024")
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",") if v]
    tail_batches = [int(v) for v in a.tail_batches.split(",") if v]
    cfg = M.encoder_config("zh")
    opt = M.make_opt(pair_bow_dim=V)
    model = M.DrlClassifier(opt, cfg, seed=0).to("cuda").train()
    optim = M.FusedAdam(model, lr=1e-5, fuse_into_backward=True)
    res = dict(seq_len=S, layers=cfg.layers, bow_dim=V, steps=a.steps, warmup=a.warmup, tail_batch_limit=ops.tail_batch_limit(opt.ec_dim, opt.e_num_class))
    res["tail"] = bench_tail(model, tail_batches, a.steps, a.warmup)
    res["step"] = bench_steps(model, optim, cfg, batches, a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
