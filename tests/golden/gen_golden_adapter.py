#!/usr/bin/env python3
"""Golden vectors of the EMNLP scripts' adapter model, made by EXECUTING the reference's own code on CPU (the style of gen_golden.py).

The `ClassDef` / `FunctionDef` nodes of `SparsemaxMultiheadAttention`, `EntmaxMultiheadAttention`, `DrlClassifier`, `MMDStatistic`,
`pdist` and `permutation_test_mat` (drl_classifier_ec_mmd_final_mul_emnlp.py) are AST-extracted at run time and exec'd with
`device = cpu`, the locally constructed HF encoders of gen_golden.py, and `entmax15` / `Sparsemax` bound to the restatement in
tests/adapter_restate.py (the `entmax` / `sparsemax` packages are not installed).  Nothing from the reference is copied.

Encoder / head weights come from `oracle.carel_oracle.init_params(seed)` and the adapter weights from
`tests.adapter_restate.adapter_params(mode, heads, seed, kscale)` -- both regenerated from frozen streams, not stored; a fixture holds
the inputs, the two 768-float queries, seeds and the reference's outputs: the state_dict key list and shapes, adapter outputs,
mu / log_var, every term and the loss, gradient slices and norms, three torch.optim.Adam(get_params()) steps and eval predictions.

    python tests/golden/gen_golden_adapter.py          # writes tests/golden/adapter_*.npz
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from gen_golden import OUT, REF, SLICE_KEYS, extract, reference_namespace, slices, to_opt_ns  # noqa: E402
from oracle import carel_oracle as O  # noqa: E402
from tests import adapter_restate as R  # noqa: E402

EMNLP = "drl_classifier_ec_mmd_final_mul_emnlp.py"


class _Sparsemax(nn.Module):
    """Stands in for `sparsemax.Sparsemax(dim)`."""

    def __init__(self, dim=-1):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        return R.sparsemax_fn(x, self.dim)


def emnlp_namespace(opt_ns, cfg):
    ns = reference_namespace(opt_ns, cfg)         # torch / nn / math / opt / the local HF encoders
    ns.update(device=torch.device("cpu"), Sparsemax=_Sparsemax, entmax15=lambda x, dim=-1: R.entmax15_fn(x, dim))
    mod = extract(os.path.join(REF, EMNLP), ["SparsemaxMultiheadAttention", "EntmaxMultiheadAttention", "DrlClassifier", "MMDStatistic",
                                             "pdist", "permutation_test_mat"])
    exec(compile(mod, "<reference:%s>" % EMNLP, "exec"), ns)
    return ns


def run_case(name, cfg, opt, mode, heads, kscale, B, S, wseed, bseed, aseed, shape="B", steps=3, iteration0=3):
    opt_ns = to_opt_ns(opt)
    opt_ns.adapter, opt_ns.head_number = mode, heads
    ns = emnlp_namespace(opt_ns, cfg)
    torch.manual_seed(1234)
    model = ns["DrlClassifier"](ns["opt"])
    P = O.init_params(cfg, opt, seed=wseed)
    A = R.adapter_params(mode, heads, seed=aseed, kscale=kscale)
    sd = model.state_dict()
    extra = [k for k in sd if k not in P and k not in A]
    assert all(("position_ids" in k) or ("token_type_ids" in k) for k in extra), extra
    model.load_state_dict({**{k: sd[k] for k in extra}, **P, **A}, strict=True)
    rs = np.random.RandomState(aseed + 1)
    q = rs.standard_normal((2, 768)).astype(np.float32)
    model.emotion_q = torch.from_numpy(q[0]).view(1, 1, 768).clone()
    model.cause_q = torch.from_numpy(q[1]).view(1, 1, 768).clone()
    batch = O.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=bseed, shape=shape)
    model.train()          # every dropout probability is 0 here
    optim = torch.optim.Adam(model.get_params(), lr=opt.vae_lr)
    keys = [k for k in model.state_dict() if not k.endswith(("position_ids", "token_type_ids"))]
    rec = dict(meta=np.array([B, S, cfg.layers, cfg.vocab_size, opt.pair_bow_dim, wseed, bseed, steps, iteration0, heads, aseed],
                             dtype=np.int64),
               mode=np.array(mode), kscale=np.float32(kscale), shape=np.array(shape), variant=np.array(cfg.variant),
               queries=q, sd_keys=np.array(keys), sd_shapes=np.array([",".join(map(str, sd[k].shape)) for k in keys]),
               versions=np.array(f"torch={torch.__version__};transformers={__import__('transformers').__version__}"))
    for k, v in batch.items():
        rec["in_" + k] = v.numpy()
    losses = []
    for s in range(steps):
        torch.manual_seed(1000 + s)
        eps_e, eps_c = torch.randn(opt.ec_dim), torch.randn(opt.ec_dim)
        rec[f"eps_e_{s}"], rec[f"eps_c_{s}"] = eps_e.numpy(), eps_c.numpy()
        torch.manual_seed(1000 + s)    # sample_prior draws eps_e then eps_c from the global stream
        loss = model(batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], batch["emo_labels"], batch["cau_labels"],
                     batch["labels"], batch["bow_reps"], iteration0 + s)
        if s == 0:     # per-term capture with the reference's own sub-modules on the same noise
            with torch.no_grad():
                h = model.encoder(batch["input_ids"], attention_mask=batch["attention_masks"],
                                  token_type_ids=batch["token_type_ids"]).last_hidden_state
                a_e, p_e = model.emotion_adapter(model.emotion_q.expand(B, 1, 768), h, h)
                a_c, p_c = model.cause_adapter(model.cause_q.expand(B, 1, 768), h, h)
                a_e, a_c = a_e.squeeze(1), a_c.squeeze(1)
                mu_e, lv_e = model.get_emotion_emb(a_e)
                mu_c, lv_c = model.get_cause_emb(a_c)
                z_e, z_c = mu_e + eps_e * torch.exp(lv_e), mu_c + eps_c * torch.exp(lv_c)
                z = torch.cat((z_e, z_c), 1)
                rec["adapter_e"], rec["adapter_c"] = a_e.numpy(), a_c.numpy()
                rec["support_e"] = (p_e.reshape(B, -1) > 0).sum(-1).numpy().astype(np.int64)
                rec["support_c"] = (p_c.reshape(B, -1) > 0).sum(-1).numpy().astype(np.int64)
                rec["mu_e"], rec["lv_e"], rec["mu_c"], rec["lv_c"] = (t.numpy() for t in (mu_e, lv_e, mu_c, lv_c))
                rec["t_emo"] = model.get_emotion_mul_loss(z_e, batch["emo_labels"]).numpy()
                rec["t_cau"] = model.get_cause_mul_loss(z_c, batch["cau_labels"]).numpy()
                rec["t_mmd"] = ns["MMDStatistic"](B, B)(z_e, z_c, [0.1]).numpy()
                pl = model.get_pair_mul_loss(z, batch["labels"])
                rec["t_pair"] = np.float32(pl if isinstance(pl, int) else pl.numpy())
                w = model.get_annealed_weight(iteration0, opt.ec_kl_lambda)
                rec["t_kl_e"] = (w * model.get_kl_loss(mu_e, lv_e)).numpy()
                rec["t_kl_c"] = (w * model.get_kl_loss(mu_c, lv_c)).numpy()
                rec["t_rec"] = model.get_reconstruct_loss(nn.Softmax(dim=1)(model.decoder(z)), batch["bow_reps"]).numpy()
        optim.zero_grad()
        loss.backward()
        if s == 0:
            named = dict(model.named_parameters())
            for k in SLICE_KEYS:
                if k in named:
                    g = named[k].grad
                    rec["g_" + k] = slices(g if g is not None else torch.zeros_like(named[k]))
                    rec["gn_" + k] = np.float32(0.0 if g is None else g.norm().item())
        optim.step()
        losses.append(loss.item())
    rec["losses"] = np.array(losses, dtype=np.float64)
    named = dict(model.named_parameters())
    for k in SLICE_KEYS:
        if k in named:
            rec["w_" + k] = slices(named[k])
    model.eval()
    torch.manual_seed(77)
    rec["pred_eps_e"], rec["pred_eps_c"] = torch.randn(opt.ec_dim).numpy(), torch.randn(opt.ec_dim).numpy()
    torch.manual_seed(77)
    with torch.no_grad():
        rec["preds"] = np.array(model.get_pair_preds(batch["input_ids"], batch["attention_masks"], batch["token_type_ids"]),
                                dtype=np.float32)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print(name, "losses", losses, "supports e", rec["support_e"].tolist(), "c", rec["support_c"].tolist())


if __name__ == "__main__":
    torch.set_num_threads(8)
    zh = O.EncoderConfig(layers=2, vocab_size=1000)
    en = O.EncoderConfig(layers=2, vocab_size=1200, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)
    nodrop = dict(dropout=0.0)
    run_case("adapter_zh_entmax", zh, O.Opt(pair_bow_dim=513, **nodrop), "entmax", 4, 1.0, B=8, S=128, wseed=12, bseed=22, aseed=31)
    run_case("adapter_zh_entmax_narrow", zh, O.Opt(pair_bow_dim=513, **nodrop), "entmax", 4, 20.0, B=8, S=128, wseed=12, bseed=22,
             aseed=32)
    run_case("adapter_zh_sparsemax", zh, O.Opt(pair_bow_dim=513, **nodrop), "sparsemax", 4, 4.0, B=8, S=128, wseed=12, bseed=22, aseed=33)
    run_case("adapter_zh_raw", zh, O.Opt(pair_bow_dim=513, **nodrop), "raw", 4, 1.0, B=8, S=128, wseed=12, bseed=22, aseed=34)
    run_case("adapter_en_entmax", en, O.Opt(language="en", pair_bow_dim=257, **nodrop), "entmax", 4, 1.0, B=8, S=128, wseed=14,
             bseed=24, aseed=35)
