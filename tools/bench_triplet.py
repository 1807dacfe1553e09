#!/usr/bin/env python3
"""Device time of one batch triplet loss call (forward + gradient w.r.t. the embeddings, H = 768) through the C ABI:
carel_triplet_loss (csrc/triplet_family.hip: four launches) per mode at B = 16 .. 512, with the old one-workgroup
carel_triplet_semihard beside it at B <= 64, the two ALTERNATING call by call in one process.  Every call is timed with its own
pair of device events; the median of --calls calls after --warmup warm-up calls per shape is reported.

    python tools/bench_triplet.py [--calls 200] [--warmup 20] [--batch 16,512]       # one JSON line per (B, kernel)
    rocprofv3 --kernel-trace --stats -d out/triplet_trace -- python tools/bench_triplet.py --batch 512 --calls 50   # per-kernel times at one size
    python tools/bench_triplet.py --fit [--steps 10]                   # one training step at B = 128, S = 128, 12 layers, and the loss's share

--fit times the body of SentenceTransformer.fit()'s loop written out by hand (model forward, loss, backward(), FusedAdamW.step() with
default arguments, zero_grad()) on one resident batch, so that the loss call can be bracketed with events; it does not call fit():
no scheduler, no data loader, no collate.
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
from carel_vae_amd import sentence_transformer as S  # noqa: E402

H = 768
MODES = ("semihard", "all", "hard", "hard_soft")


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3                                    # microseconds


def bench_calls(calls, warmup, batches):
    lib = L.load()
    for B in batches:
        g = torch.Generator().manual_seed(B)
        emb = torch.randn((B, H), generator=g).cuda()
        labels = torch.randint(0, max(2, B // 8), (B,), generator=g).to(torch.int32).cuda()
        loss, demb = torch.empty(1, device="cuda"), torch.empty_like(emb)
        work = torch.empty(lib.carel_triplet_workspace_floats(B), device="cuda")
        fns = {}
        for mode, name in enumerate(MODES):
            a = L.TripletArgs()
            a.emb, a.labels, a.batch, a.hidden, a.mode, a.distance, a.margin = emb.data_ptr(), labels.data_ptr(), B, H, mode, 0, 5.0
            a.loss_out, a.demb, a.work = loss.data_ptr(), demb.data_ptr(), work.data_ptr()
            fns[name] = (lambda a=a: L.check(lib.carel_triplet_loss(C.byref(a), L.current_stream())))
        if B <= 64:
            fns["semihard_old_kernel"] = lambda: L.check(lib.carel_triplet_semihard(emb.data_ptr(), labels.data_ptr(), B, H, 5.0, loss.data_ptr(),
                                                                                    demb.data_ptr(), L.current_stream()))
        times = {k: [] for k in fns}
        for i in range(warmup + calls):                                 # the kernels alternate call by call: same clocks, same neighbours
            for k, fn in fns.items():
                t = timed(fn)
                if i >= warmup:
                    times[k].append(t)
        for k, v in times.items():
            v.sort()
            print(json.dumps({"B": B, "kernel": k, "median_us": round(statistics.median(v), 2), "p10_us": round(v[len(v) // 10], 2),
                              "p90_us": round(v[len(v) * 9 // 10], 2), "calls": len(v)}), flush=True)


def bench_fit(steps, warmup):
    B, S_ = 128, 128
    model = S.SentenceTransformer(M.encoder_config("zh"), max_seq_length=S_, seed=0).to("cuda")
    g = torch.Generator().manual_seed(1)
    feats = {"input_ids": torch.randint(1000, 20000, (B, S_), generator=g), "attention_mask": torch.ones((B, S_), dtype=torch.long),
             "token_type_ids": torch.zeros((B, S_), dtype=torch.long), "seq_lengths": [S_] * B}
    labels = torch.randint(0, 16, (B,), generator=g)
    loss_mod = S.losses.BatchAllTripletLoss(model=model, margin=10)
    optim = S.FusedAdamW(model, lr=2e-5)
    model.train(True)
    step_us, loss_us = [], []
    for i in range(warmup + steps):
        t0, t1, t2, t3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        t0.record()
        emb = model(feats)["sentence_embedding"]
        t1.record()
        loss = loss_mod.batch_all_triplet_loss(labels, emb)
        t2.record()
        loss.backward()
        optim.step()
        optim.zero_grad()
        t3.record()
        t3.synchronize()
        if i >= warmup:
            step_us.append(t0.elapsed_time(t3) * 1e3)
            loss_us.append(t1.elapsed_time(t2) * 1e3)
    print(json.dumps({"hand_written_fit_loop_body": "B=128 S=128 12 layers BatchAllTripletLoss", "step_median_us": round(statistics.median(step_us), 1),
                      "loss_forward_and_gradient_median_us": round(statistics.median(loss_us), 1),
                      "loss_share": round(statistics.median(loss_us) / statistics.median(step_us), 5), "steps": len(step_us)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", default="16,32,64,128,256,512", help="comma-separated batch sizes (1..512)")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    if a.fit:
        bench_fit(a.steps, min(a.warmup, 3))
    else:
        bench_calls(a.calls, a.warmup, [int(b) for b in a.batch.split(",")])


if __name__ == "__main__":
    main()
