#!/usr/bin/env python3
"""What the element-weighted content losses (opt.bow_loss, carel_en_tail_losses_bow) cost: the dense training step of the zh
three-space model at 12 layers, B = 64, S = 128, V = 23 771 (dropout on, the six fused optimisers, the reference's six backward
calls) with bow_loss off and on, and the three tail calls (latents, losses, backward) of each alone.
Protocol of tools/bench_large_batch.py: ONE process, the two legs interleaved step by step (same clocks, same neighbours), median of
20 after 5 warm-ups each, timed with events.

    python tools/bench_en_bow.py [--steps 20] [--warmup 5] [--legs off,on]

On a tree without the option (the commit before it) only the `off` leg exists and only it is run, so the same tool gives the figure
the `off` leg is compared with.  Prints one JSON line: step_ms / tail_us / tail_share per leg, and on_minus_off_us for both.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from carel_vae_amd import _lib as L  # noqa: E402
from carel_vae_amd import drl_classifier as M  # noqa: E402
from carel_vae_amd import drl_classifier_en as ME  # noqa: E402
from carel_vae_amd import ops  # noqa: E402
from carel_vae_amd.data import synthetic_ecpe_batch  # noqa: E402

B, S, V = 64, 128, 23771
HAS_OPTION = hasattr(ME, "bow_loss_config")


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def make_leg(on, cfg):
    opt = ME.make_opt(language="zh", pair_bow_dim=V, **(dict(bow_loss=True) if on else {}))
    model = ME.DrlClassifier(opt, cfg, seed=0).to("cuda").train()
    assert bool(getattr(model, "bow_loss", False)) is on
    return model, model.make_fused_optimizers(fuse_into_backward=True)


def step(model, opts, b, i):
    cd_e, cd_c, ed, ecd, cad, ced, vae = model(b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"],
                                               b["labels"], b["bow_reps"], i % 41)
    opts[0].zero_grad(); (cd_e + cd_c).backward(retain_graph=True)        # noqa: E702   the reference's order
    opts[1].zero_grad(); ed.backward(retain_graph=True)                  # noqa: E702
    opts[3].zero_grad(); ecd.backward(retain_graph=True)                 # noqa: E702
    opts[2].zero_grad(); cad.backward(retain_graph=True)                 # noqa: E702
    opts[4].zero_grad(); ced.backward(retain_graph=True)                 # noqa: E702
    opts[5].zero_grad(); vae.backward()                                  # noqa: E702
    for o in opts:
        o.step()


def tail_calls(model):
    """The three tail calls on the arguments of the model's last step (its own weights, buffers and gradient destinations)."""
    lib, c = L.load(), model._last_call
    one = torch.ones(1, device="cuda")

    def losses():
        if getattr(model, "bow_loss", False):
            ops.en_tail_losses_bow(c.ta, ops.en_bow_args(c.buf.bow_work))
        else:
            L.check(lib.carel_en_tail_losses(C.byref(c.ta), L.current_stream()), "carel_en_tail_losses")
    return dict(latents=lambda: L.check(lib.carel_en_tail_latents(C.byref(c.ta), L.current_stream()), "carel_en_tail_latents"),
                losses=losses,
                backward=lambda: L.check(lib.carel_en_tail_backward(C.byref(c.ta), one.data_ptr(), L.current_stream()), "carel_en_tail_backward"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default="off,on")
    a = ap.parse_args()
    legs = [n for n in a.legs.split(",") if n in ("off", "on") and (n == "off" or HAS_OPTION)]
    cfg = M.encoder_config("zh")
    batch = {k: v.cuda() for k, v in synthetic_ecpe_batch(B, S, cfg.vocab_size, V, seed=3, shape="A", binary_emotion=True).items()}
    built = {n: make_leg(n == "on", cfg) for n in legs}
    times = {n: [] for n in legs}
    for i in range(a.warmup + a.steps):
        for n, (model, opts) in built.items():
            torch.cuda.synchronize()
            ms = timed(lambda: step(model, opts, batch, i))
            if i >= a.warmup:
                times[n].append(ms)
    tails = {n: tail_calls(built[n][0]) for n in legs}
    tail_t = {n: {k: [] for k in tails[n]} for n in legs}
    for i in range(a.warmup + a.steps):
        for n in legs:
            for k, fn in tails[n].items():
                torch.cuda.synchronize()
                us = 1000.0 * timed(fn)
                if i >= a.warmup:
                    tail_t[n][k].append(us)
    res = dict(batch=B, seq_len=S, layers=cfg.layers, bow_dim=V, steps=a.steps, warmup=a.warmup, has_option=HAS_OPTION)
    for n in legs:
        med = statistics.median(times[n])
        t = {k + "_us": round(statistics.median(v), 2) for k, v in tail_t[n].items()}
        t["total_us"] = round(sum(t.values()), 2)
        res[n] = dict(step_ms_median=round(med, 4), step_ms_min=round(min(times[n]), 4), step_ms_max=round(max(times[n]), 4), tail=t,
                      tail_share=round(t["total_us"] / (1000.0 * med), 4))
    if "off" in res and "on" in res:
        res["on_minus_off_us"] = dict(step=round(1000.0 * (res["on"]["step_ms_median"] - res["off"]["step_ms_median"]), 1),
                                      tail_losses=round(res["on"]["tail"]["losses_us"] - res["off"]["tail"]["losses_us"], 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
