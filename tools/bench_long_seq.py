"""Long-sequence measurements: one JSON line per case.

    python tools/bench_long_seq.py [--iters 20] [--warmup 5] [--no-sdpa] [--no-step]

  attn      carel_attention_fwd / _bwd of one layer at B*S = 8 192 tokens for S = 128 (the one-workgroup-per-(sample, head) kernels)
            and 256 / 384 / 512 (csrc/attention_long.hip); TFLOP/s from the shapes: forward 4*B*12*S*S*64, backward 2.5x that
            (the five products of a flash-style backward; the S = 128 kernel does four, its rate is still quoted on the same count)
  sdpa      torch.nn.functional.scaled_dot_product_attention on the same bf16 q, k, v (forward, forward + backward): a yardstick
  step      DrlClassifier training step (12 layers, dense and ECPE-shaped packed lengths) at max_len 256 (B 32) and 512 (B 16, 32)
Times are device events around `iters` back-to-back calls after `warmup` untimed ones, median of 5 such windows."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carel_vae_amd import _lib as L                     # noqa: E402
from carel_vae_amd import drl_classifier as M           # noqa: E402
from oracle import carel_oracle as O                    # noqa: E402

NH, HD, H = 12, 64, 768


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    ms.sort()
    return ms[2]


def attn_cases(args):
    lib = L.load()
    for S in (128, 256, 384, 512):
        B = 8192 // S
        g = torch.Generator().manual_seed(S)
        qkv = (torch.randn((B * S, 3 * H), generator=g)).cuda().bfloat16()
        ctx = torch.empty((B * S, H), device="cuda", dtype=torch.bfloat16)
        lse = torch.empty((B, NH, S), device="cuda")
        dctx = torch.randn((B * S, H), generator=g).cuda().bfloat16()
        dqkv = torch.empty((B * S, 3 * H), device="cuda", dtype=torch.bfloat16)
        nws = lib.carel_attention_bwd_workspace_bytes(B, S, 0)
        ws = torch.empty(max(nws, 1), device="cuda", dtype=torch.uint8)
        a = L.AttnArgs()
        a.qkv, a.ctx, a.lse, a.dctx, a.dqkv = qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx.data_ptr(), dqkv.data_ptr()
        a.batch, a.seq_len, a.heads, a.head_dim = B, S, NH, HD
        a.workspace, a.workspace_bytes = ws.data_ptr(), nws
        st = L.current_stream()
        fwd = lambda: L.check(lib.carel_attention_fwd(C.byref(a), st), "fwd")
        bwd = lambda: L.check(lib.carel_attention_bwd(C.byref(a), st), "bwd")
        fwd()
        t_f = timed(fwd, args.iters, args.warmup)
        t_b = timed(bwd, args.iters, args.warmup)
        fl = 4.0 * B * NH * S * S * HD
        print(json.dumps(dict(case="attn", S=S, B=B, kernel="short" if S <= 128 else "long", fwd_us=round(t_f * 1e3, 2),
                              fwd_tflops=round(fl / (t_f * 1e-3) / 1e12, 1), bwd_us=round(t_b * 1e3, 2),
                              bwd_tflops=round(2.5 * fl / (t_b * 1e-3) / 1e12, 1),
                              bwd_frac_of_2p5pf=round(2.5 * fl / (t_b * 1e-3) / 2.5e15, 3))), flush=True)
        if args.sdpa:
            q, k, v = (qkv.view(B, S, 3, NH, HD)[:, :, i].transpose(1, 2).contiguous().requires_grad_(True) for i in range(3))
            sd = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v)
            go = torch.randn((B, NH, S, HD), device="cuda", dtype=torch.bfloat16)
            t_sf = timed(sd, args.iters, args.warmup)
            t_sfb = timed(lambda: torch.autograd.grad(sd(), (q, k, v), go), args.iters, args.warmup)
            print(json.dumps(dict(case="sdpa", S=S, B=B, fwd_us=round(t_sf * 1e3, 2), fwd_tflops=round(fl / (t_sf * 1e-3) / 1e12, 1),
                                  fwd_bwd_us=round(t_sfb * 1e3, 2))), flush=True)
        del qkv, ctx, lse, dctx, dqkv, ws
        torch.cuda.empty_cache()


def step_cases(args):
    cfg = O.EncoderConfig(layers=12)
    opt = O.Opt(dropout=0.1)
    for S, B in ((256, 32), (512, 16), (512, 32)):             # 8 192, 8 192 and 16 384 rows dense
        for shape in ("A", "B"):
            batch = O.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=1, shape=shape)
            model = M.DrlClassifier(M.make_opt(**vars(opt)), M.encoder_config("zh"))
            model.load_state_dict(O.init_params(cfg, opt, seed=0))
            model.to("cuda").train()
            optim = M.FusedAdam(model, lr=1e-5)
            b = {k: v.cuda() for k, v in batch.items()}

            def step():
                loss = model(b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"],
                             b["bow_reps"], 3)
                optim.zero_grad()
                loss.backward()
                optim.step()
            t = timed(step, max(2, args.iters // 4), 2)
            tokens = int(batch["attention_masks"].sum())
            print(json.dumps(dict(case="step", max_len=S, batch=B, shape=shape, packed=model._last_call.pack is not None,
                                  attended_tokens=tokens, step_ms=round(t, 3), pairs_per_s=round(B / (t * 1e-3), 1))), flush=True)
            del model, optim
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-sdpa", dest="sdpa", action="store_false")
    ap.add_argument("--no-step", dest="step", action="store_false")
    args = ap.parse_args()
    L.check(L.load().carel_init(0), "carel_init")
    attn_cases(args)
    if args.step:
        step_cases(args)


if __name__ == "__main__":
    main()
