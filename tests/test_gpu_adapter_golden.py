"""Adapter mode against the reference's own EMNLP classes: tests/golden/adapter_*.npz (gen_golden_adapter.py) -- bf16 path within the
constants of test_gpu_model.py, the fp32 debug forward at 1e-5, gradient slices, and three Adam steps."""
import os

import numpy as np
import pytest
import torch

from carel_vae_amd import drl_classifier as M
from oracle import carel_oracle as O
from tests import adapter_restate as R
from tests.test_gpu_model import (TERMS, TOL_FP32_DEBUG, TOL_KL_BF16, TOL_LATENT_BF16, TOL_LOSS_BF16, TOL_LOSS_OVER_SCALE,
                                  TOL_TERM_BF16, WEIGHTS)

pytestmark = pytest.mark.gpu

CASES = ["adapter_zh_entmax", "adapter_zh_entmax_narrow", "adapter_zh_sparsemax", "adapter_zh_raw", "adapter_en_entmax"]
LATENTS = ("adapter_e", "adapter_c", "mu_e", "lv_e", "mu_c", "lv_c")


def relnorm(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    batch = {k[3:]: torch.from_numpy(z[k]).cuda() for k in z.files if k.startswith("in_")}
    return z, batch


def build(z):
    B, S, Lr, vocab, V, wseed, bseed, steps, it0, heads, aseed = (int(v) for v in z["meta"])
    mode, kscale = str(z["mode"]), float(z["kscale"])
    if str(z["variant"]) == "roberta":
        cfg = O.EncoderConfig(layers=Lr, vocab_size=vocab, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)
        opt = O.Opt(language="en", pair_bow_dim=V, dropout=0.0)
    else:
        cfg, opt = O.EncoderConfig(layers=Lr, vocab_size=vocab), O.Opt(pair_bow_dim=V, dropout=0.0)
    mcfg = M.encoder_config("en" if cfg.variant == "roberta" else "zh", vocab_size=cfg.vocab_size, max_pos=cfg.max_pos,
                            type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps, layers=cfg.layers, hidden_dropout=0.0, attn_dropout=0.0)
    model = M.DrlClassifier(M.make_opt(**vars(opt), adapter=mode, head_number=heads), mcfg)
    model.load_state_dict({**O.init_params(cfg, opt, seed=wseed), **R.adapter_params(mode, heads, seed=aseed, kscale=kscale)})
    q = torch.from_numpy(z["queries"])
    model.emotion_q, model.cause_q = q[0].view(1, 1, 768).clone(), q[1].view(1, 1, 768).clone()
    return model.to("cuda").train(), opt, it0, steps


def call(batch, it):
    return (batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], batch["emo_labels"], batch["cau_labels"],
            batch["labels"], batch["bow_reps"], it)


def check(out, z, lat_tol, term_tol, kl_tol, loss_tol, loss_scale_tol):
    for k in LATENTS:
        assert relnorm(out[k], torch.from_numpy(z[k])) < lat_tol, (k, relnorm(out[k], torch.from_numpy(z[k])))
    for k in TERMS:
        r = float(z["t_" + k])
        tol = kl_tol if k.startswith("kl") else term_tol
        assert abs(float(out[k]) - r) <= tol * max(abs(r), 1e-3), (k, float(out[k]), r)
    scale = sum(abs(WEIGHTS[k] * float(z["t_" + k])) for k in TERMS)
    ref, dl = float(z["losses"][0]), abs(float(out["loss"]) - float(z["losses"][0]))
    assert dl <= loss_scale_tol * scale, (dl, scale)
    if abs(ref) >= 0.1 * scale:
        assert dl <= loss_tol * abs(ref), (float(out["loss"]), ref)


@pytest.mark.parametrize("name", CASES)
def test_bf16_forward_and_gradients_vs_reference(golden_dir, name):
    z, batch = load(golden_dir, name)
    model, opt, it0, _ = build(z)
    eps = (torch.from_numpy(z["eps_e_0"]), torch.from_numpy(z["eps_c_0"]))
    outs = []
    for varlen in (True, False):          # varlen / cls_only_last set by the caller change nothing: adapter mode runs dense
        model.varlen = model.cls_only_last = varlen
        model.set_noise(*eps)
        outs.append(model.forward_terms(*call(batch, it0)))
        assert model._last_call.pack is None and model._last_call.cls is None
    for k in LATENTS + TERMS + ("loss",):
        assert torch.equal(outs[0][k], outs[1][k]), k
    check(outs[0], z, TOL_LATENT_BF16, TOL_TERM_BF16, TOL_KL_BF16, TOL_LOSS_BF16, TOL_LOSS_OVER_SCALE)
    # gradients: direction agreement of the reference's fp32 slices (the bound of test_gradients_vs_oracle)
    model.varlen = True
    model.set_noise(*eps)
    model(*call(batch, it0)).backward()
    named = dict(model.named_parameters())
    checked = 0
    for k in z.files:
        if not k.startswith("g_"):
            continue
        pk = k[2:]
        f = named[pk].grad.detach().cpu().reshape(-1)
        if float(z["gn_" + pk]) <= 1e-7:                      # the pooler (grad None in the reference): exactly zero here
            if pk.startswith("encoder.pooler"):
                assert float(f.abs().max()) == 0.0
            continue
        if pk.endswith("key.bias"):      # exact gradient 0 (softmax shift invariance): both sides are rounding noise (test_gradients_vs_oracle)
            continue
        n = 64
        step = max(1, f.numel() // n)
        got = torch.cat((f[:n], f[-n:], f[::step][:n])).numpy()
        den = np.linalg.norm(z[k])
        if named[pk].numel() == 1:       # a one-element head bias: a sum of signed per-sample residuals that can nearly cancel; judged on
            den = max(den, float(z["gn_" + pk[:-len("bias")] + "weight"]))      # the scale of its own weight's gradient (same residuals)
        if den > 1e-9:
            assert np.linalg.norm(got - z[k]) / den < 8e-2, pk
            checked += 1
    assert checked >= 20
    assert model.emotion_adapter.in_proj_weight.grad is None
    pad = model.cfg.pad_id                  # padding_idx: the padded positions the adapters read send nothing into the pad rows
    assert float(named["encoder.embeddings.word_embeddings.weight"].grad[pad].abs().max()) == 0.0
    if model.cfg.roberta:
        assert float(named["encoder.embeddings.position_embeddings.weight"].grad[pad].abs().max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_fp32_debug_forward_vs_reference(golden_dir, name):
    z, batch = load(golden_dir, name)
    model, opt, it0, _ = build(z)
    model.debug_fp32 = True
    model.set_noise(torch.from_numpy(z["eps_e_0"]), torch.from_numpy(z["eps_c_0"]))
    out = model.forward_terms(*call(batch, it0))
    check(out, z, TOL_FP32_DEBUG, TOL_FP32_DEBUG, TOL_FP32_DEBUG, TOL_FP32_DEBUG, TOL_FP32_DEBUG)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["adapter_zh_entmax", "adapter_zh_sparsemax", "adapter_zh_raw"])
def test_three_adam_steps_vs_reference(golden_dir, name, fused):
    z, batch = load(golden_dir, name)
    model, opt, it0, steps = build(z)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    queries = (model.emotion_q.clone(), model.cause_q.clone())
    optim = M.FusedAdam(model, lr=opt.vae_lr) if fused else torch.optim.Adam(model.get_params(), lr=opt.vae_lr)
    losses = []
    for s in range(steps):
        model.set_noise(torch.from_numpy(z[f"eps_e_{s}"]), torch.from_numpy(z[f"eps_c_{s}"]))
        loss = model(*call(batch, it0 + s))
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(float(loss))
    scale = sum(abs(WEIGHTS[k] * float(z["t_" + k])) for k in TERMS)
    assert np.abs(np.array(losses) - z["losses"]).max() < 6e-3 * scale, (losses, z["losses"])
    sd = model.state_dict()
    for k in z.files:                        # the bound of test_three_step_adam_trajectory
        if k.startswith("w_"):
            pk = k[2:]
            f = sd[pk].detach().cpu().reshape(-1)
            n = 64
            step = max(1, f.numel() // n)
            got = torch.cat((f[:n], f[-n:], f[::step][:n])).numpy()
            d = np.abs(got - z[k])
            assert d.max() <= 2 * steps * opt.vae_lr * 1.01, pk
            if not pk.endswith("key.bias"):
                assert (d <= 1.2e-5).mean() >= 0.97, (pk, float((d <= 1.2e-5).mean()))
    frozen = ["encoder.pooler.dense.weight", "encoder.pooler.dense.bias", "emotion_mu.weight", "emotion_log_var.bias", "cause_mu.weight",
              "cause_log_var.weight"] + model._adapter_names
    for k in frozen:
        assert torch.equal(sd[k], before[k]), k
    assert torch.equal(model.emotion_q, queries[0]) and torch.equal(model.cause_q, queries[1])
