"""Restatement of the adversarial (GAN) disentangler of drl_classifier_ec_gan.py for the tests: the two one-logit adversaries on the
detached sampled embeddings, the entropy terms the vae loss adds, and the three-optimiser step.  Everything else of that script's
forward is the `none` tail with the one-logit BCE emotion head, taken from oracle.carel_oracle (imported, not edited).  Works in
float32 (against the fixture written by tests/golden/gen_golden_gan.py) and in float64 (the yardstick of the kernel tests).

    ec_disc_preds = sigmoid(ec_disc(dropout(z_c.detach())))   scored against the EMOTION labels   (:222-225, :430-442)
    ce_disc_preds = sigmoid(ce_disc(dropout(z_e.detach())))   scored against the CAUSE labels     (:231-234, :444-456)
    disc loss     = BCELoss(preds, y (1 - ls) + ls / 1)                                            (:458-470)
    entropy       = mean_b sum_k p log(p + epsilon)                                                 (:472-477)
    vae loss      = w_ecce (ec_ent + ce_ent) + w_ec (emo + cau) + w_pair pair + kl_e + kl_c + rec  (:275-279)
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE

SITE_EC_DISC, SITE_CE_DISC = 103, 104          # the two dropout sites of carel_gan_disc (after the tail's 100..102)
GAN_KEYS = ("ec_disc.weight", "ec_disc.bias", "ce_disc.weight", "ce_disc.bias")
GROUPS = (("ec_disc.weight", "ec_disc.bias"), ("ce_disc.weight", "ce_disc.bias"))
LOSS_NAMES = ("ec_disc_loss", "ce_disc_loss", "vae")

# parser defaults of the script (:30-57)
DEFAULTS = dict(max_len=128, ec_num_class=1, pair_num_class=1, ec_dim=24, con_dim=384, pair_bow_dim=23771, bert_dim=768,
                kl_ann_iterations=20000, epochs=10, batch_size=64, ec_kl_lambda=0.03, con_kl_lambda=0.03, label_smoothing=0.1,
                ecce_adv_loss_weight=1.0, ec_mul_loss_weight=10.0, pair_mul_loss_weight=25.0, dropout=0.5, epsilon=1e-8, adv_lr=0.003,
                vae_lr=1e-5, self_iteration=50, self_epochs=10, self_strategy="random")


def gan_opt(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return SimpleNamespace(**d)


def oracle_opt(opt) -> O.Opt:
    """The carel_oracle.Opt under which tail_forward(disentangle="none", emotion_head="bce") is this script's tail: both heads
    weighted by ec_mul_loss_weight."""
    return O.Opt(e_num_class=1, c_num_class=1, pair_num_class=1, ec_dim=opt.ec_dim, kl_ann_iterations=opt.kl_ann_iterations,
                 ec_kl_lambda=opt.ec_kl_lambda, label_smoothing=opt.label_smoothing, emo_mul_loss_weight=opt.ec_mul_loss_weight,
                 cau_mul_loss_weight=opt.ec_mul_loss_weight, pair_mul_loss_weight=opt.pair_mul_loss_weight, dropout=opt.dropout,
                 epsilon=opt.epsilon, vae_lr=opt.vae_lr, pair_bow_dim=opt.pair_bow_dim)


def init_gan_params(ec_dim, seed=0):
    """nn.Linear-style uniform(+-1/sqrt(fan_in)) for ec_disc / ce_disc (:168-169), numpy RandomState stream."""
    rs = np.random.RandomState(seed)
    bound = 1.0 / math.sqrt(ec_dim)
    return {k: torch.from_numpy(rs.uniform(-bound, bound, size=(1, ec_dim) if k.endswith("weight") else (1,)).astype(np.float32))
            for k in GAN_KEYS}


def init_params(cfg, opt, seed):
    """Every tensor of the script's state_dict: carel_oracle.init_params for the shared part, init_gan_params(seed + 1) for the rest."""
    return {**O.init_params(cfg, oracle_opt(opt), seed=seed), **init_gan_params(opt.ec_dim, seed + 1)}


def state_dict_keys(cfg, opt):
    """Registration order of the script (:156-180): ... cause_log_var, ec_disc, ce_disc, emotion_classifier ..."""
    keys = list(O.param_shapes(cfg, oracle_opt(opt)))
    i = keys.index("cause_log_var.bias") + 1
    return keys[:i] + list(GAN_KEYS) + keys[i:]


def disc_terms(P, z_e, z_c, emo_labels, cau_labels, label_smoothing, epsilon, p_drop=0.0, seed=None, row_offset=0):
    """The four scalars of the two adversaries, in the dtype of P / z (float64 for the kernel tests); z_e / z_c are detached here as in
    the script, so the result is differentiable with respect to the four discriminator tensors only."""
    B, D = z_e.shape
    dt = z_e.dtype
    out = {}
    for name, src, y, site in (("ec", z_c, emo_labels, SITE_EC_DISC), ("ce", z_e, cau_labels, SITE_CE_DISC)):
        x = src.detach()
        m = O.dropout_scale_mask(seed, site, (B, D), p_drop, row_offset)
        if m is not None:
            x = x * m.to(dt)
        p = torch.sigmoid(x @ P[name + "_disc.weight"].to(dt).t() + P[name + "_disc.bias"].to(dt))
        t = y.reshape(-1, 1).to(dt) * (1 - label_smoothing) + label_smoothing / 1
        out[name + "_disc_loss"] = O.bce_prob(p, t).mean()
        out[name + "_entropy"] = (p * torch.log(p + epsilon)).sum(dim=1).mean()
    return out


def forward_terms(P, batch, iteration, cfg, opt, eps_e, eps_c, train=False, seed=None, quant=None):
    """The script's forward (:182-281): the three returned losses under LOSS_NAMES plus every term."""
    oo = oracle_opt(opt)
    pooled = O.encoder_forward(P, batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], cfg, train=train, seed=seed,
                               quant=quant)
    out = O.tail_forward(P, pooled, batch["emo_labels"], batch["cau_labels"], batch["labels"], batch["bow_reps"], iteration, oo,
                         eps_e, eps_c, train=train, seed=seed, disentangle="none", emotion_head="bce")
    out.update(disc_terms(P, out["z_e"], out["z_c"], batch["emo_labels"], batch["cau_labels"], opt.label_smoothing, opt.epsilon,
                          opt.dropout if train else 0.0, seed))
    out["vae"] = out["loss"] + opt.ecce_adv_loss_weight * (out["ec_entropy"] + out["ce_entropy"])
    out["pooled"] = pooled
    return out


def loss_and_grads(P, batch, iteration, cfg, opt, eps_e, eps_c, **kw):
    """The three backward calls of the step (:790-798) and the gradient each optimiser then sees: a discriminator's own loss, plus --
    because zero_grad clears one group only -- the entropy share of the vae loss, which reaches the discriminators alone."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = forward_terms(leaf, batch, iteration, cfg, opt, eps_e, eps_c, **kw)
    grads = {}
    for keys, loss in zip(GROUPS, (out["ec_disc_loss"], out["ce_disc_loss"])):
        for k, g in zip(keys, torch.autograd.grad(loss, [leaf[k] for k in keys], retain_graph=True)):
            grads[k] = g
    allk = list(GAN_KEYS) + O.optimised_keys(cfg, oracle_opt(opt))
    for k, g in zip(allk, torch.autograd.grad(out["vae"], [leaf[k] for k in allk], allow_unused=True)):
        if g is not None:
            grads[k] = grads[k] + g if k in grads else g
    return {k: v.detach() for k, v in out.items()}, grads


def train_step(P, batch, iteration, cfg, opt, states, eps_e, eps_c, **kw):
    """One iteration of the loop (:784-802) with the optimisers of the script body (:903-908): RMSprop(adv_lr) for each adversary,
    Adam(vae_lr) for get_params()[2].  states: three carel_oracle.AdamState."""
    out, grads = loss_and_grads(P, batch, iteration, cfg, opt, eps_e, eps_c, **kw)
    P = dict(P)
    for i, keys in enumerate(GROUPS):
        P = OE.rmsprop_step(P, grads, list(keys), states[i], lr=opt.adv_lr)
    P = O.adam_step(P, grads, O.optimised_keys(cfg, oracle_opt(opt)), states[2], lr=opt.vae_lr)
    return P, out, grads


def synthetic_batch(B, S, cfg, V, seed=1, shape="B"):
    """ECPE-shaped batch with binary float emotion AND cause labels (both values present, so the adversaries see both classes)."""
    return OE.synthetic_batch(B, S, cfg, V, seed=seed, shape=shape)
