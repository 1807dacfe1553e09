#!/usr/bin/env python3
"""What opt.disentangle == "gan" costs per training step: the dense B = 64, S = 128, 12-layer step with fused optimisers, the `none`
model with the one-logit BCE head and the gan model interleaved step by step in ONE process (same clocks, same neighbours); median
of 20 steps after 5 warm-ups each, timed with events.  The difference should be the gan step's three extra launches (gan_disc and
the two RMSprop updates) plus the four small gradient-share launches of its backward calls.

    python tools/bench_gan.py [--steps 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d out/gan_trace -- python tools/bench_gan.py      # per-kernel times (gan_disc_kernel, rmsprop)
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
    a = ap.parse_args()
    gopt = M.make_gan_opt(pair_bow_dim=V)
    nopt = M.make_opt(pair_bow_dim=V, e_num_class=1, disentangle="none", emotion_head="bce", emo_mul_loss_weight=gopt.ec_mul_loss_weight,
                      cau_mul_loss_weight=gopt.ec_mul_loss_weight, pair_mul_loss_weight=gopt.pair_mul_loss_weight, epochs=gopt.epochs)
    cfg = M.encoder_config("zh")
    batch = {k: v.cuda() for k, v in synthetic_ecpe_batch(B, S, cfg.vocab_size, V, seed=3, shape="A", binary_emotion=True).items()}
    args = lambda emo, i: (batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], emo, batch["cau_labels"],   # noqa: E731
                           batch["labels"], batch["bow_reps"], i % 41)
    emo_f, emo_i = batch["emo_labels"].float(), batch["emo_labels"].long()

    none = M.DrlClassifier(nopt, cfg, seed=0).to("cuda").train()
    none_opt = M.FusedAdam(none, lr=nopt.vae_lr, fuse_into_backward=True)
    gan = M.DrlClassifier(gopt, cfg, seed=0).to("cuda").train()
    gan_opts = gan.make_fused_optimizers(fuse_into_backward=True)

    def step_none(i):
        loss = none(*args(emo_i, i))
        none_opt.zero_grad()
        loss.backward()
        none_opt.step()

    def step_gan(i):                      # drl_classifier_ec_gan.py:784-802
        ec_d, ce_d, vae = gan(*args(emo_f, i))
        gan_opts[0].zero_grad(); ec_d.backward(retain_graph=True)          # noqa: E702
        gan_opts[1].zero_grad(); ce_d.backward(retain_graph=True)          # noqa: E702
        gan_opts[2].zero_grad(); vae.backward()                            # noqa: E702
        for o in gan_opts:
            o.step()

    times = {"none_bce": [], "gan": []}
    for i in range(a.warmup + a.steps):
        for name, fn in (("none_bce", step_none), ("gan", step_gan)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn(i)
            t1.record()
            t1.synchronize()
            if i >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    res = {k + "_ms_median": round(statistics.median(v), 4) for k, v in times.items()}
    res.update({k + "_ms_min": round(min(v), 4) for k, v in times.items()})
    res["delta_ms_median"] = round(res["gan_ms_median"] - res["none_bce_ms_median"], 4)
    res.update(batch=B, seq_len=S, layers=cfg.layers, steps=a.steps, warmup=a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
