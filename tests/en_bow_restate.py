"""Restatement, for the tests, of the tail of the reference's three-space model with the ELEMENT-WEIGHTED content losses of
drl_classifier_bow_loss.py (:245-257, :438-448, :537-550):

    con_w = sigmoid(content_classifier(dropout(z_content)))         [B, V]; a dropout draw of its own (site 120), detached
    content_disc_loss_{emo,cau} = BCELoss(weight = 1 - con_w)(softmax(content_disc(dropout(z_{e,c}))), smoothed_bow)
    content_mul_loss            = BCELoss(weight = con_w)    (softmax(content_classifier(dropout(z_content))), smoothed_bow)

Everything else (entropies, decoder, one-logit heads, KL terms, weighted sum) is the tail of drl_classifier.py /
drl_classifier_en.py.  `tail_from_latents` works in whatever dtype its inputs have: float32 against the fixtures written by
tests/golden/gen_golden_zh3.py, float64 as the yardstick of the kernel tests; weighting = "plain" is the unweighted tail (the same
arithmetic as oracle.carel_oracle_en.tail_forward, which the host test checks), "bow" the weighted one.
The encoder is oracle.carel_oracle.encoder_forward (imported, not edited), so `quant=O.bf16_round` rounds at its storage points.
"""
from typing import Dict, Optional

import torch

from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE

SITE_CON_W = 120                 # the eleventh dropped-out copy (after OE's 110..119)
LOSS_NAMES = OE.LOSS_NAMES
LAT_NAMES = ("mu_con", "lv_con", "mu_e", "lv_e", "mu_c", "lv_c")


def split_lat(lat, opt):
    """The kernel's latent layout [B, 2*con_dim + 4*ec_dim] -> the six named blocks."""
    D, Cd = opt.ec_dim, opt.con_dim
    cuts = (0, Cd, 2 * Cd, 2 * Cd + D, 2 * Cd + 2 * D, 2 * Cd + 3 * D, 2 * Cd + 4 * D)
    return {n: lat[:, cuts[i]:cuts[i + 1]] for i, n in enumerate(LAT_NAMES)}


def tail_from_latents(P, lat: Dict[str, torch.Tensor], emo_labels, cau_labels, pair_labels, bow, kl_w_ec: float, kl_w_con: float, opt,
                      eps: Dict[str, torch.Tensor], weighting: str = "bow", train: bool = False, seed: Optional[int] = None,
                      row_offset: int = 0, pos_weight=None) -> Dict[str, torch.Tensor]:
    """Everything after the six latent heads.  lat: {mu_con, lv_con, mu_e, lv_e, mu_c, lv_c}; eps: {con, e, c}.
    pos_weight: the pair term's pos_weight given explicitly (a data-parallel shard uses the global batch's); None: (B - sum y) / sum y."""
    assert weighting in ("plain", "bow")
    dt = lat["mu_e"].dtype
    B = lat["mu_e"].shape[0]
    V, ls = opt.pair_bow_dim, opt.label_smoothing
    W = {k: v.to(dt) if v.is_floating_point() else v for k, v in P.items() if not k.startswith("encoder.")}

    def lin(x, name):
        return x @ W[name + ".weight"].t() + W[name + ".bias"]
    z_con = lat["mu_con"] + eps["con"].to(dt) * torch.exp(lat["lv_con"])
    z_e = lat["mu_e"] + eps["e"].to(dt) * torch.exp(lat["lv_e"])
    z_c = lat["mu_c"] + eps["c"].to(dt) * torch.exp(lat["lv_c"])
    gen, pair_emb = torch.cat((z_e, z_c, z_con), dim=1), torch.cat((z_e, z_c), dim=1)
    pd = opt.dropout if train else 0.0

    def drop(t, site):
        m = O.dropout_scale_mask(seed, site, tuple(t.shape), pd, row_offset)
        return t if m is None else t * m.to(dt)
    emo_y, cau_y, pair_y = (y.reshape(B, -1).to(dt) for y in (emo_labels, cau_labels, pair_labels))
    bow_t = bow.to(dt) * (1 - ls) + ls / V
    ec_t = lambda y: y * (1 - ls) + ls / opt.ec_num_class     # noqa: E731

    def entropy(p):
        return (p * torch.log(p + opt.epsilon)).sum(dim=1).mean()
    if weighting == "bow":          # :245-247; nn.BCELoss(weight=w.detach()) multiplies the clamped element losses, then takes the plain mean
        con_w = torch.sigmoid(lin(drop(z_con, SITE_CON_W), "content_classifier")).detach()
        ec_w = 1 - con_w
    else:
        con_w = ec_w = torch.ones((), dtype=dt)
    p_cd_e = torch.softmax(lin(drop(z_e.detach(), OE.SITE_CDISC_E), "content_disc"), dim=1)
    p_cd_c = torch.softmax(lin(drop(z_c.detach(), OE.SITE_CDISC_C), "content_disc"), dim=1)
    cd_e, cd_c = (ec_w * O.bce_prob(p_cd_e, bow_t)).mean(), (ec_w * O.bce_prob(p_cd_c, bow_t)).mean()
    cent_e, cent_c = entropy(p_cd_e), entropy(p_cd_c)
    con_mul = (con_w * O.bce_prob(torch.softmax(lin(drop(z_con, OE.SITE_CMUL), "content_classifier"), dim=1), bow_t)).mean()
    p_ed = torch.sigmoid(lin(drop(z_con.detach(), OE.SITE_EDISC), "emotion_disc"))
    p_ec = torch.sigmoid(lin(drop(z_c.detach(), OE.SITE_ECDISC), "ec_disc"))
    ed, ecd = O.bce_prob(p_ed, ec_t(emo_y)).mean(), O.bce_prob(p_ec, ec_t(emo_y)).mean()
    ent_ed, ent_ec = entropy(p_ed), entropy(p_ec)
    emo_mul = O.bce_prob(torch.sigmoid(lin(drop(z_e, OE.SITE_EMUL), "emotion_classifier")), ec_t(emo_y)).mean()
    p_cad = torch.sigmoid(lin(drop(z_con.detach(), OE.SITE_CAUDISC), "cause_disc"))
    p_ce = torch.sigmoid(lin(drop(z_e.detach(), OE.SITE_CEDISC), "ce_disc"))
    cad, ced = O.bce_prob(p_cad, ec_t(cau_y)).mean(), O.bce_prob(p_ce, ec_t(cau_y)).mean()
    ent_cad, ent_ce = entropy(p_cad), entropy(p_ce)
    cau_mul = O.bce_prob(torch.sigmoid(lin(drop(z_c, OE.SITE_CAUMUL), "cause_classifier")), ec_t(cau_y)).mean()
    xp = lin(drop(pair_emb, OE.SITE_PAIR), "pair_classifier")
    sy = pair_y.sum()
    pair = O.bce_logits_posw(xp, ec_t(pair_y), (B - sy) / sy if pos_weight is None else pos_weight).mean()

    def kl(mu, lv):
        return (-0.5 * (1 + lv - lv.exp() - mu.pow(2)).sum(dim=1)).mean()
    kl_e, kl_c, kl_con = kl_w_ec * kl(lat["mu_e"], lat["lv_e"]), kl_w_ec * kl(lat["mu_c"], lat["lv_c"]), kl_w_con * kl(lat["mu_con"], lat["lv_con"])
    rec = O.bce_prob(torch.softmax(lin(gen, "decoder"), dim=1), bow_t).mean()
    vae = (opt.con_adv_loss_weight * (cent_e + cent_c) + opt.ec_adv_loss_weight * (ent_ed + ent_cad)
           + opt.ecce_adv_loss_weight * (ent_ec + ent_ce) + opt.ec_mul_loss_weight * (emo_mul + cau_mul)
           + opt.con_mul_loss_weight * con_mul + opt.pair_mul_loss_weight * pair + kl_e + kl_c + kl_con + rec)
    return dict(content_disc_emo=cd_e, content_disc_cau=cd_c, emotion_disc=ed, ec_disc=ecd, cause_disc=cad, ce_disc=ced, vae=vae,
                cent_e=cent_e, cent_c=cent_c, ent_ed=ent_ed, ent_cad=ent_cad, ent_ec=ent_ec, ent_ce=ent_ce, emo_mul=emo_mul,
                cau_mul=cau_mul, con_mul=con_mul, pair=pair, kl_e=kl_e, kl_c=kl_c, kl_con=kl_con, rec=rec, z=gen, pair_logit=xp,
                con_w=con_w, **lat)


def kl_weights(iteration, opt):
    if iteration < opt.kl_ann_iterations:
        return OE.kl_anneal_weight(iteration, opt, opt.ec_kl_lambda), OE.kl_anneal_weight(iteration, opt, opt.con_kl_lambda)
    return 1.0, 1.0


def tail_forward(P, pooled, emo_labels, cau_labels, pair_labels, bow, iteration, opt, eps, weighting="bow", **kw):
    """From pooler_output: the six latent heads, then tail_from_latents."""
    heads = dict(mu_con="content_mu", lv_con="content_log_var", mu_e="emotion_mu", lv_e="emotion_log_var", mu_c="cause_mu", lv_c="cause_log_var")
    lat = {n: pooled @ P[h + ".weight"].t().to(pooled.dtype) + P[h + ".bias"].to(pooled.dtype) for n, h in heads.items()}
    kl_e, kl_con = kl_weights(iteration, opt)
    return tail_from_latents(P, lat, emo_labels, cau_labels, pair_labels, bow, kl_e, kl_con, opt, eps, weighting=weighting, **kw)


def forward_terms(P, batch, iteration, cfg, opt, eps, weighting="bow", train=False, seed=None, quant: O.Quant = None, row_offset=0):
    pooled = O.encoder_forward(P, batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], cfg, train=train, seed=seed,
                               row_offset=row_offset, quant=quant)
    out = tail_forward(P, pooled, batch["emo_labels"], batch["cau_labels"], batch["labels"], batch["bow_reps"], iteration, opt, eps,
                       weighting=weighting, train=train, seed=seed, row_offset=row_offset)
    out["pooled"] = pooled
    return out


def loss_and_grads(P, batch, iteration, cfg, opt, eps, weighting="bow", **kw):
    """The six backward calls of the step and the gradients each optimiser then sees (as oracle.carel_oracle_en.loss_and_grads)."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = forward_terms(leaf, batch, iteration, cfg, opt, eps, weighting=weighting, **kw)
    groups = OE.group_keys(cfg, opt)
    disc_losses = [out["content_disc_emo"] + out["content_disc_cau"], out["emotion_disc"], out["cause_disc"], out["ec_disc"], out["ce_disc"]]
    grads: Dict[str, torch.Tensor] = {}
    for keys, loss in zip(groups[:5], disc_losses):
        for k, g in zip(keys, torch.autograd.grad(loss, [leaf[k] for k in keys], retain_graph=True)):
            grads[k] = g
    allk = [k for g in groups for k in g]
    for k, g in zip(allk, torch.autograd.grad(out["vae"], [leaf[k] for k in allk], allow_unused=True)):
        if g is not None:
            grads[k] = grads[k] + g if k in grads else g
    return {k: v.detach() for k, v in out.items()}, grads


def train_step(P, batch, iteration, cfg, opt, states, eps, weighting="bow", **kw):
    """One iteration with the optimisers the scripts build: RMSprop(adv_lr) for the five discriminators, Adam(vae_lr) for the rest."""
    out, grads = loss_and_grads(P, batch, iteration, cfg, opt, eps, weighting=weighting, **kw)
    P = dict(P)
    for i, keys in enumerate(OE.group_keys(cfg, opt)):
        P = OE.rmsprop_step(P, grads, keys, states[i], lr=opt.adv_lr) if i < 5 else O.adam_step(P, grads, keys, states[i], lr=opt.vae_lr)
    return P, out, grads
