#!/usr/bin/env python3
"""Golden vectors for the adversarial (GAN) ablation (drl_classifier_ec_gan.py), produced by EXECUTING the reference's own
`DrlClassifier` class (AST-extracted at run time, nothing copied) on CPU around a locally constructed 2-layer BertModel.

The update sequence below -- two discriminator backward calls with retain_graph, the vae backward, then the three optimiser
steps -- is the procedure of the reference's training loop (:784-802) with the optimisers its script body builds (RMSprop for the
two adversaries, Adam for the rest, :903-908); every model call in it is reference code.  Weights come from
tests/gan_restate.init_params (numpy RandomState), so the fixture holds inputs, noise and expected outputs only.  The parser
defaults are read out of the script's own `parser.add_argument` calls (AST literals; the script is not run).

    python tests/golden/gen_golden_gan.py         # writes tests/golden/gan_small.npz; does nothing where the reference is absent
"""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import carel_oracle as O  # noqa: E402
from tests import gan_restate as R  # noqa: E402
import gen_golden as G  # noqa: E402

SCRIPT = os.path.join(G.REF, "drl_classifier_ec_gan.py")
HEAD_KEYS = list(R.GAN_KEYS) + ["emotion_classifier.weight", "emotion_classifier.bias", "cause_classifier.weight", "cause_classifier.bias",
                                "pair_classifier.weight", "pair_classifier.bias", "decoder.weight", "decoder.bias"]
ENC_KEYS = [k for k in G.SLICE_KEYS if k.startswith("encoder.")]
RECORDED_DEFAULTS = ("max_len", "ec_num_class", "pair_num_class", "ec_dim", "pair_bow_dim", "bert_dim", "kl_ann_iterations", "epochs",
                     "batch_size", "ec_kl_lambda", "label_smoothing", "ecce_adv_loss_weight", "ec_mul_loss_weight", "pair_mul_loss_weight",
                     "dropout", "epsilon", "adv_lr", "vae_lr", "self_iteration", "self_epochs", "self_strategy")


def parser_defaults():
    """name -> default of every `parser.add_argument('--name', ..., default=<literal>)` of the script."""
    out = {}
    for node in ast.walk(ast.parse(open(SCRIPT, encoding="utf8").read())):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args:
            name = ast.literal_eval(node.args[0]).lstrip("-")
            for kw in node.keywords:
                if kw.arg == "default":
                    out[name] = ast.literal_eval(kw.value)
    return out


def gan_namespace(opt_ns, cfg):
    import math
    import transformers

    def make_bert():
        c = transformers.BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                                    num_attention_heads=cfg.heads, intermediate_size=cfg.intermediate,
                                    max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.ln_eps,
                                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu")
        c._attn_implementation = "eager"
        return transformers.BertModel(c)

    class _Stub:
        def from_pretrained(self, *a, **k):      # local construction, nothing fetched
            return make_bert()

    ns = dict(torch=torch, nn=nn, math=math, opt=opt_ns, np=np, BertModel=_Stub())
    mod = G.extract(SCRIPT, ["DrlClassifier"])
    exec(compile(mod, "<reference:drl_classifier_ec_gan.py>", "exec"), ns)
    return ns


def main():
    if not os.path.exists(SCRIPT):
        print("reference script not found: nothing written")
        return
    defaults = parser_defaults()
    cfg = O.EncoderConfig(layers=2, vocab_size=900)
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    B, S, wseed, bseed, steps = 16, 128, 71, 81, 3
    ref_opt = types.SimpleNamespace(**vars(opt))
    ns = gan_namespace(ref_opt, cfg)
    torch.manual_seed(1234)
    model = ns["DrlClassifier"](ref_opt)
    P = R.init_params(cfg, opt, wseed)
    sd = model.state_dict()
    extra = [k for k in sd if k not in P]
    assert all(("position_ids" in k) or ("token_type_ids" in k) for k in extra), extra
    assert not [k for k in P if k not in sd]
    model.load_state_dict({**{k: sd[k] for k in extra}, **P})
    batch = R.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=bseed, shape="B")
    assert 0 < float(batch["emo_labels"].sum()) < B and 0 < float(batch["cau_labels"].sum()) < B, "the batch must hold both labels"
    model.train()
    named = dict(model.named_parameters())
    ids = {id(p): k for k, p in named.items()}
    groups = [list(g) for g in model.get_params()]
    keys = [k for k in sd if k not in extra]
    rec = dict(meta=np.array([B, S, cfg.layers, cfg.vocab_size, opt.pair_bow_dim, wseed, bseed, steps], dtype=np.int64),
               versions=np.array(f"torch={torch.__version__};transformers={__import__('transformers').__version__}"),
               sd_keys=np.array(keys), sd_shapes=np.array(json.dumps([list(sd[k].shape) for k in keys])),
               group_keys=np.array(json.dumps([[ids[id(p)] for p in g] for g in groups])),
               defaults=np.array(json.dumps({k: defaults[k] for k in RECORDED_DEFAULTS})))
    opts = [torch.optim.RMSprop(groups[0], lr=opt.adv_lr), torch.optim.RMSprop(groups[1], lr=opt.adv_lr),
            torch.optim.Adam(groups[2], lr=opt.vae_lr)]                                              # :903-908
    for k, v in batch.items():
        rec["in_" + k] = v.numpy()
    for s in range(steps):
        torch.manual_seed(5000 + s)                       # sample_prior order: emotion, cause (:213-214)
        rec[f"eps_e_{s}"] = torch.randn(opt.ec_dim).numpy()
        rec[f"eps_c_{s}"] = torch.randn(opt.ec_dim).numpy()
        torch.manual_seed(5000 + s)
        losses = model(batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], batch["emo_labels"].view(-1, 1),
                       batch["cau_labels"].view(-1, 1), batch["labels"].view(-1, 1), batch["bow_reps"], 7 + s)
        rec[f"losses_{s}"] = np.array([float(v.item()) for v in losses], dtype=np.float64)
        ec_d, ce_d, vae = losses
        opts[0].zero_grad(); ec_d.backward(retain_graph=True)                 # noqa: E702   :790-798, same order
        opts[1].zero_grad(); ce_d.backward(retain_graph=True)                 # noqa: E702
        opts[2].zero_grad(); vae.backward()                                  # noqa: E702
        if s == 1:
            for k in HEAD_KEYS + ENC_KEYS:
                if named[k].grad is not None:
                    rec["g_" + k] = G.slices(named[k].grad)
                    rec["gn_" + k] = np.float32(named[k].grad.norm().item())
        for o in opts:
            o.step()
    for k in HEAD_KEYS + ENC_KEYS:
        rec["w_" + k] = G.slices(named[k])
    # get_pair_preds (:283-300): rounded probabilities as a nested list, emotion noise before cause noise
    model.eval()
    torch.manual_seed(5100)
    rec["pp_eps_e"], rec["pp_eps_c"] = torch.randn(opt.ec_dim).numpy(), torch.randn(opt.ec_dim).numpy()
    torch.manual_seed(5100)
    with torch.no_grad():
        rec["pp_preds"] = np.array(model.get_pair_preds(batch["input_ids"], batch["attention_masks"], batch["token_type_ids"]), dtype=np.float32)
    np.savez_compressed(os.path.join(G.OUT, "gan_small.npz"), **rec)
    print({k: v for k, v in rec.items() if k.startswith("losses_")})


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
