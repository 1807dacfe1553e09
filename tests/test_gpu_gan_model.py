"""opt.disentangle == "gan" on the HIP path: the model of drl_classifier_ec_gan.py (two adversaries on the sampled embeddings, three
optimisers) against (a) the fixture written by the reference's own class (tests/golden/gen_golden_gan.py), (b) the `none` model
with the BCE head, bit for bit, (c) its own gradient images, (d) the bf16-emulating restatement on a ragged batch, packed and
padded, (e) the training driver and (f) a checkpoint round trip."""
import os

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import training as T
from oracle import carel_oracle as O
from tests import gan_restate as R

pytestmark = pytest.mark.gpu

CFG = O.EncoderConfig(layers=2, vocab_size=900)
DISC = ("ec_disc", "ce_disc")
# a gradient accumulated by separate additions (or scaled after the fact) against the multiple it equals in exact arithmetic: a few fp32
# roundings of partial sums, relative to the tensor's norm (17 x 2^-24)
TOL_SUM_CHAIN = 1e-6


def build(opt, wseed, cfg=CFG, train_dropout=False, disentangle="gan"):
    mcfg = M.encoder_config("zh", vocab_size=cfg.vocab_size, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps,
                            layers=cfg.layers, hidden_dropout=cfg.hidden_dropout if train_dropout else 0.0,
                            attn_dropout=cfg.attn_dropout if train_dropout else 0.0)
    P = R.init_params(cfg, opt, wseed)
    if disentangle == "gan":
        model = M.DrlClassifier(M.make_gan_opt(**vars(opt)), mcfg)
    else:           # the `none` model with the one-logit BCE head and this script's weights
        model = M.DrlClassifier(M.make_opt(**{**vars(R.oracle_opt(opt)), "disentangle": "none", "emotion_head": "bce"}), mcfg)
        P = {k: v for k, v in P.items() if k not in R.GAN_KEYS}
    model.load_state_dict(P)
    model.to("cuda")
    return model, P


def load(golden_dir, name="gan_small"):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, batch


def call(batch, it):
    b = {k: v.cuda() for k, v in batch.items()}
    return (b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], it)


def relnorm(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def gslice(t, n=64):
    f = t.detach().cpu().reshape(-1)
    step = max(1, f.numel() // n)
    return torch.cat((f[:n], f[-n:], f[::step][:n])).numpy()


def reference_step(losses, opts):
    """The backward / zero_grad sequence of the reference's loop (drl_classifier_ec_gan.py:790-798)."""
    ec_d, ce_d, vae = losses
    opts[0].zero_grad(); ec_d.backward(retain_graph=True)                 # noqa: E702
    opts[1].zero_grad(); ce_d.backward(retain_graph=True)                 # noqa: E702
    opts[2].zero_grad(); vae.backward()                                  # noqa: E702


def stock_optimizers(model, opt):
    gp = model.get_params()
    return [torch.optim.RMSprop(gp[0], lr=opt.adv_lr), torch.optim.RMSprop(gp[1], lr=opt.adv_lr), torch.optim.Adam(gp[2], lr=opt.vae_lr)]


# ------------------------------------------------------------------------------------------------ (a) the fixture
@pytest.mark.parametrize("fused", [False, True])
def test_three_steps_follow_the_reference(golden_dir, fused):
    """Losses of every step, the discriminators' gradients at step 1 and the weights after three steps against the reference class; the
    constants of tests/test_gpu_en_adv.py for the same three comparisons (fp32 reference, bf16 encoder here)."""
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    z, batch = load(golden_dir)
    B, S, Lr, vocab, V, wseed, bseed, steps = (int(v) for v in z["meta"])
    model, P = build(opt, wseed)
    model.train()
    opts = list(model.make_fused_optimizers(fuse_into_backward=True)) if fused else stock_optimizers(model, opt)
    if fused:
        assert [type(o).__name__ for o in opts] == ["FusedRMSprop", "FusedRMSprop", "FusedAdam"]
    named = dict(model.named_parameters())
    for s in range(steps):
        model.set_noise(torch.from_numpy(z[f"eps_e_{s}"]), torch.from_numpy(z[f"eps_c_{s}"]))
        losses = model(*call(batch, 7 + s))
        assert len(losses) == 3
        reference_step(losses, opts)
        if s == 1:
            for g in DISC:
                got, ref = gslice(named[g + ".weight"].grad), z["g_" + g + ".weight"]
                print("grad", g, relnorm(torch.from_numpy(got), torch.from_numpy(ref)))
                assert relnorm(torch.from_numpy(got), torch.from_numpy(ref)) <= 1.5e-2, g
                gb, rb = float(named[g + ".bias"].grad), float(z["g_" + g + ".bias"][0])
                assert abs(gb - rb) <= 4e-2 * abs(rb) + 2e-2, (g, gb, rb)       # one-logit bias: a signed mean that nearly cancels
        for o in opts:
            o.step()
        got = np.array([float(v.detach()) for v in losses])
        print("losses", s, got, z[f"losses_{s}"])
        np.testing.assert_allclose(got, z[f"losses_{s}"], rtol=2e-2, atol=2e-3, err_msg=f"step {s}")
    sd = model.state_dict()
    for k in z.files:
        if k.startswith("w_"):
            pk = k[2:]
            lr = 10 * opt.adv_lr if pk in R.GAN_KEYS else opt.vae_lr       # an RMSprop step is up to lr / sqrt(1 - alpha)
            d = np.abs(gslice(sd[pk]) - z[k])
            assert d.max() <= 2 * steps * lr * 1.01, pk
            if not pk.endswith("key.bias"):
                assert (d <= 1.2 * lr).mean() >= 0.95, (pk, float((d <= 1.2 * lr).mean()))
    P0 = R.init_params(CFG, opt, wseed)
    for n in ("emotion_mu.weight", "cause_log_var.bias"):            # latent heads never move
        assert torch.equal(sd[n].cpu(), P0[n])
    for n in R.GAN_KEYS:
        assert not torch.equal(sd[n].cpu(), P0[n]), n


def test_forward_terms_eval_forward_and_pair_preds(golden_dir):
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    z, batch = load(golden_dir)
    wseed = int(z["meta"][5])
    model, P = build(opt, wseed)
    model.train()
    eps_e, eps_c = torch.from_numpy(z["eps_e_0"]), torch.from_numpy(z["eps_c_0"])
    model.set_noise(eps_e, eps_c)
    t = model.forward_terms(*call(batch, 7))
    ref = R.forward_terms(P, batch, 7, CFG, opt, eps_e, eps_c, quant=O.bf16_round)
    for n in ("ec_disc_loss", "ce_disc_loss", "ec_entropy", "ce_entropy"):
        r = float(ref[n])
        assert abs(float(t[n]) - r) <= 3e-3 * max(abs(r), 1e-3) + 1e-6, (n, float(t[n]), r)
    np.testing.assert_allclose([float(t["ec_disc_loss"]), float(t["ce_disc_loss"]), float(t["vae_and_classifier_loss"])], z["losses_0"],
                               rtol=2e-2, atol=1e-3)
    model.eval()
    with torch.no_grad():
        model.set_noise(eps_e, eps_c)
        losses = model(*call(batch, 7))
    assert len(losses) == 3 and not losses[2].requires_grad
    np.testing.assert_allclose(np.array([float(v) for v in losses]), z["losses_0"], rtol=2e-2, atol=1e-3)
    b = {k: v.cuda() for k, v in batch.items()}
    model.set_noise(torch.from_numpy(z["pp_eps_e"]), torch.from_numpy(z["pp_eps_c"]))
    prob = model.pair_probabilities(b["input_ids"], b["attention_masks"], b["token_type_ids"]).cpu()
    model.set_noise(torch.from_numpy(z["pp_eps_e"]), torch.from_numpy(z["pp_eps_c"]))
    preds = model.get_pair_preds(b["input_ids"], b["attention_masks"], b["token_type_ids"])
    assert isinstance(preds, list) and len(preds) == prob.numel() and all(p[0] in (0.0, 1.0) for p in preds)
    clear = ((prob - 0.5).abs() > 2e-2).numpy()               # bf16 encoder: a probability near 1/2 may round either way
    assert clear.sum() >= prob.numel() // 2
    assert np.array_equal(np.array(preds).reshape(-1)[clear], z["pp_preds"].reshape(-1)[clear])


# ------------------------------------------------------------------------------------------------ (b) exact
@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_non_discriminator_gradients_are_those_of_the_none_model_bit_for_bit(golden_dir, dropout):
    """The two .detach() calls: nothing from either adversary reaches the latents or the encoder, and the entropy terms reach the
    adversaries only.  With equal weights, noise and seeds every other gradient is bit-identical to the `none` + BCE-head model's, and
    the vae loss is that model's loss plus ecce_adv_loss_weight (ec_ent + ce_ent)."""
    opt = R.gan_opt(pair_bow_dim=211, dropout=dropout, ecce_adv_loss_weight=3.0)
    z, batch = load(golden_dir)
    wseed = int(z["meta"][5])
    eps_e, eps_c = torch.from_numpy(z["eps_e_1"]), torch.from_numpy(z["eps_c_1"])
    res = {}
    for mode in ("gan", "none"):
        model, _ = build(opt, wseed, train_dropout=dropout > 0, disentangle=mode)
        model.train()
        model.set_noise(eps_e, eps_c)
        b = dict(batch)
        if mode == "none":
            b["emo_labels"] = batch["emo_labels"].long()         # the two-space scripts' integer label; the BCE head reads it as 0 / 1
        out = model(*call(b, 8))
        loss = out[2] if mode == "gan" else out
        loss.backward()
        torch.cuda.synchronize()
        res[mode] = (float(loss.detach()), model._last_call.seed, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()},
                     {k: float(v) for k, v in model.last_terms().items()}, model)
    (lg, sg, gg, tg, mg), (ln, sn, gn, tn, _) = res["gan"], res["none"]
    assert sg == sn
    assert tg == tn                                                # every term of the tail, bit for bit
    n = 0
    for k, g in gn.items():
        assert g is not None and gg[k] is not None, k
        assert torch.equal(g, gg[k]), k
        n += 1
    assert n == len(gg) - 4
    gt = mg._last_call.gan_terms.cpu()
    want = np.float32(ln) + np.float32(3.0) * (gt[2].numpy() + gt[3].numpy())
    print("vae", lg, float(want))
    assert abs(lg - float(want)) <= 4 * 6e-8 * abs(float(want))      # fp32 rounding of one multiply and two adds
    # the vae loss alone still reaches the adversaries: weighted entropy image
    for g in DISC:
        assert gg[g + ".weight"] is not None and float(gg[g + ".weight"].abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ (c) shares
def _images(model):
    """(own, entropy) images of both discriminators from the last forward, keyed by parameter name."""
    out = {}
    for i in range(2):
        for k in R.GAN_KEYS:
            o = model._offs[k] - model._disc_lo
            out[(i, k)] = model._disc_img[i][o:o + model._named[k].numel()].reshape(model._named[k].shape).clone()
    return out


def test_upstream_gradients_scale_each_share(golden_dir):
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    z, batch = load(golden_dir)
    wseed = int(z["meta"][5])
    model, P = build(opt, wseed)
    model.train()
    eps_e, eps_c = torch.from_numpy(z["eps_e_0"]), torch.from_numpy(z["eps_c_0"])
    named = dict(model.named_parameters())

    def fresh():
        for p in model.parameters():
            p.grad = None
        model.set_noise(eps_e, eps_c)
        return model(*call(batch, 7))

    # the reference's call order: own image + ecce_adv_loss_weight (= 1) x entropy image, exactly
    losses = fresh()
    reference_step(losses, stock_optimizers(model, opt))
    img = _images(model)
    for k in R.GAN_KEYS:
        assert torch.equal(named[k].grad, img[(0, k)] + img[(1, k)]), k
    # the images against the fp32 restatement on the kernel's own z (bf16 encoder upstream, so z itself is taken from the device)
    zc = model._last_call.buf.z.detach().cpu().double()
    leaf = {k: P[k].double().clone().requires_grad_(True) for k in R.GAN_KEYS}
    t = R.disc_terms(leaf, zc[:, :opt.ec_dim], zc[:, opt.ec_dim:], batch["emo_labels"].double(), batch["cau_labels"].double(),
                     opt.label_smoothing, opt.epsilon)
    for name in DISC:
        for i, term in ((0, name + "_loss"), (1, name.split("_")[0] + "_entropy")):
            for k, g in zip((name + ".weight", name + ".bias"), torch.autograd.grad(t[term], [leaf[name + ".weight"], leaf[name + ".bias"]],
                                                                                   retain_graph=True)):
                np.testing.assert_allclose(img[(i, k)].cpu().double().numpy(), g.numpy(), rtol=1e-4, atol=1e-5, err_msg=(term, k))
    # single losses: only their own discriminator gets a gradient; powers of two scale exactly
    losses = fresh()
    (2.0 * losses[0]).backward()
    assert torch.equal(named["ec_disc.weight"].grad, 2.0 * img[(0, "ec_disc.weight")])
    assert named["ce_disc.weight"].grad is None and named["decoder.weight"].grad is None
    losses = fresh()
    (-0.5 * losses[1]).backward()
    assert torch.equal(named["ce_disc.bias"].grad, -0.5 * img[(0, "ce_disc.bias")])
    assert named["ec_disc.weight"].grad is None and named["encoder.pooler.dense.weight"].grad is None
    # a mix, with accumulation inside one backward and across two
    losses = fresh()
    (4.0 * losses[0] - 2.0 * losses[1] + 0.25 * losses[2]).backward()
    assert torch.equal(named["ec_disc.weight"].grad, 4.0 * img[(0, "ec_disc.weight")] + 0.25 * img[(1, "ec_disc.weight")])
    assert torch.equal(named["ce_disc.weight"].grad, -2.0 * img[(0, "ce_disc.weight")] + 0.25 * img[(1, "ce_disc.weight")])
    dec = named["decoder.weight"].grad.clone()
    losses2 = fresh()
    losses2[2].backward()
    assert relnorm(dec, 0.25 * named["decoder.weight"].grad) < TOL_SUM_CHAIN
    first = {k: named[k].grad.clone() for k in ("ec_disc.weight", "decoder.weight", "encoder.encoder.layer.0.output.dense.weight")}
    model.set_noise(eps_e, eps_c)
    model._fwd_count -= 1
    losses3 = model(*call(batch, 7))                               # no zero_grad: everything accumulates like torch
    (losses3[0] + losses3[2]).backward()
    assert torch.equal(named["ec_disc.weight"].grad, (first["ec_disc.weight"] + img[(0, "ec_disc.weight")]) + img[(1, "ec_disc.weight")])
    for k in ("decoder.weight", "encoder.encoder.layer.0.output.dense.weight"):
        assert relnorm(named[k].grad, 2.0 * first[k]) < TOL_SUM_CHAIN, k
    # a weight other than one: to fp32 rounding of the product
    opt3 = R.gan_opt(pair_bow_dim=211, dropout=0.0, ecce_adv_loss_weight=3.0)
    model3, _ = build(opt3, wseed)
    model3.train()
    model3.set_noise(eps_e, eps_c)
    l3 = model3(*call(batch, 7))
    reference_step(l3, stock_optimizers(model3, opt3))
    img3 = _images(model3)
    for k in R.GAN_KEYS:
        want = img3[(0, k)].double() + 3.0 * img3[(1, k)].double()
        assert float((dict(model3.named_parameters())[k].grad.double() - want).abs().max()) <= 2e-7 * float(want.abs().max()), k


# ------------------------------------------------------------------------------------------------ (d) packed = padded
def test_packed_equals_padded_on_a_ragged_batch():
    """The criteria of tests/test_gpu_packed_sweep.py (its T = 1792 case: 64 ragged samples, one word id per token, three layers)
    applied to the packed and to the padded run of the gan model: a second run gives the same bits; loss terms, every parameter
    gradient, every touched word row, latent row and pooled row against the bf16-emulating restatement at that file's bounds; the
    adversaries' terms and gradients at the same bounds."""
    from tests import test_gpu_packed_sweep as PS
    from tests.test_gpu_model import TOL_GRAD_BF16_EMU, TOL_KL_BF16, TOL_LOSS_OVER_SCALE, TOL_TERM_BF16
    cfg = O.EncoderConfig(layers=3)
    opt = R.gan_opt(dropout=0.0)
    oo = R.oracle_opt(opt)
    Tn = 1792
    batch, lens = PS.packed_batch(Tn, cfg, oo, seed=Tn)
    rs = np.random.RandomState(11)
    batch["emo_labels"] = torch.from_numpy((rs.uniform(size=(PS.B, 1)) < 0.5).astype(np.float32))
    g = torch.Generator().manual_seed(Tn)
    eps_e, eps_c = torch.randn(opt.ec_dim, generator=g), torch.randn(opt.ec_dim, generator=g)
    model, P = build(opt, 0, cfg=cfg)
    model.train()

    def run():
        model.set_noise(eps_e, eps_c)
        for p in model.parameters():
            p.grad = None
        losses = model(*call(batch, 3))
        c = model._last_call
        reference_step(losses, stock_optimizers(model, opt))
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
        terms = {k: float(v) for k, v in model.last_terms().items()}
        terms.update({n: float(c.gan_terms[i]) for i, n in enumerate(("ec_disc_loss", "ce_disc_loss", "ec_entropy", "ce_entropy"))})
        return [float(v) for v in losses], terms, grads, c.buf.lat[:PS.B].detach().cpu().clone(), c.buf.pooled[:PS.B].detach().cpu().clone(), c

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    out, grads = R.loss_and_grads(P, batch, 3, cfg, opt, eps_e, eps_c, quant=O.bf16_hip)
    lat_ref = torch.cat((out["mu_e"], out["lv_e"], out["mu_c"], out["lv_c"]), 1)
    # per-sample magnitudes of the one-logit bias gradients (as the sweep holds the head biases)
    Pb = dict(P)
    for k in ("ec_disc.bias", "ce_disc.bias"):
        Pb[k] = P[k].expand(PS.B, -1).clone().requires_grad_(True)
    tb = R.disc_terms(Pb, out["z_e"], out["z_c"], batch["emo_labels"], batch["cau_labels"], opt.label_smoothing, opt.epsilon)
    (tb["ec_disc_loss"] + tb["ce_disc_loss"] + opt.ecce_adv_loss_weight * (tb["ec_entropy"] + tb["ce_entropy"])).backward()
    bias_scale = {k: float(Pb[k].grad.double().abs().sum()) for k in ("ec_disc.bias", "ce_disc.bias")}
    weights = dict(emo=opt.ec_mul_loss_weight, cau=opt.ec_mul_loss_weight, pair=opt.pair_mul_loss_weight, kl_e=1.0, kl_c=1.0, rec=1.0,
                   ec_entropy=opt.ecce_adv_loss_weight, ce_entropy=opt.ecce_adv_loss_weight)
    res = {}
    for varlen in (True, False):        # (the model is local to this test: nothing to restore)
        model.varlen = varlen
        losses, terms, got, lat, pooled, c = run()
        assert (c.pack is not None) == varlen and (not varlen or (c.pack.n_tokens == Tn and c.pack.t_eff == int(lens.sum())))
        model._fwd_count -= 1
        losses2, _, got2, lat2, _, c2 = run()
        assert c2.seed == c.seed and losses2 == losses and torch.equal(lat2, lat)
        for k, v in got.items():
            assert torch.equal(got2[k], v), (varlen, k)
        for k in weights:
            r = float(out[k])
            tol = TOL_KL_BF16 if k.startswith("kl") else TOL_TERM_BF16
            assert abs(terms[k] - r) <= tol * max(abs(r), 1e-3), (varlen, k, terms[k], r)
        for i, k in enumerate(("ec_disc_loss", "ce_disc_loss")):
            assert abs(losses[i] - float(out[k])) <= TOL_TERM_BF16 * abs(float(out[k])), (varlen, k)
        scale = sum(abs(w * float(out[k])) for k, w in weights.items())
        assert abs(losses[2] - float(out["vae"])) <= TOL_LOSS_OVER_SCALE * scale, (varlen, losses[2], float(out["vae"]), scale)
        shared = {k: v for k, v in grads.items() if k not in R.GAN_KEYS}
        qk, rest = PS.grad_errors({k: v for k, v in got.items() if k not in R.GAN_KEYS}, shared, P, batch, out, oo, eps_e, eps_c,
                                  disentangle="none", emotion_head="bce")
        PS.assert_grads(qk, rest, varlen)
        for k in R.GAN_KEYS:
            den = float(grads[k].double().norm()) if k.endswith("weight") else max(float(grads[k].double().norm()), 0.1 * bias_scale[k])
            err = float((got[k].double() - grads[k].double()).norm()) / den
            print("disc grad", varlen, k, err)
            assert err <= TOL_GRAD_BF16_EMU, (varlen, k, err)
        touched = torch.zeros(cfg.vocab_size, dtype=torch.bool)
        touched[batch["input_ids"][batch["attention_masks"] == 1]] = True
        word_rows = PS.rows_relerr(got[PS.WORD][touched], grads[PS.WORD][touched])
        assert torch.equal(got[PS.WORD].abs().sum(1) > 0, touched), varlen
        assert word_rows.max() <= PS.TOL_WORD_ROW, (varlen, float(word_rows.max()))
        assert PS.rows_relerr(lat, lat_ref).max() <= PS.TOL_LATENT_ROW, varlen
        assert PS.rows_relerr(pooled, out["pooled"]).max() <= PS.TOL_POOLED_ROW, varlen
        res[varlen] = (losses, terms, got)
    # packed against padded directly, at the bounds tests/test_gpu_model.py::test_token_packing_equals_padded_computation uses (not
    # bitwise: the packed batch takes the split-K GEMM path, whose fp32 summation order differs)
    (l1, t1, g1), (l0, t0, g0) = res[True], res[False]
    for k in t0:
        assert abs(t0[k] - t1[k]) <= 1e-3 * max(abs(t0[k]), 1e-3), (k, t0[k], t1[k])
    for a_, b_ in zip(l0, l1):
        assert abs(a_ - b_) <= 1e-3 * max(abs(a_), 1e-3)
    # (key biases: analytically zero.  The one-logit biases are signed sums of one term per sample that can nearly cancel; the sweep's
    # criteria above hold them on the scale of their terms, a plain relative norm would not be meaningful for them)
    one_logit = PS.HEAD_BIASES + ("ec_disc.bias", "ce_disc.bias")
    worst = max(relnorm(g1[k], g0[k]) for k in g0 if float(g0[k].norm()) > 1e-6 and not k.endswith("key.bias") and k not in one_logit)
    print("packed vs padded worst", worst)
    assert worst < 2e-2, worst


# ------------------------------------------------------------------------------------------------ (e) the driver
def test_train_driver_end_to_end_with_three_optimisers(tmp_path):
    """drl_classifier_ec_gan.py's loop (:784-811) through train(): the adversaries on fused RMSprop, the rest on fused Adam inside
    backward, float emotion labels of all ones (:83, :133), the running loss the sum of the three losses."""
    from tests.test_gpu_training import _loaders
    torch.manual_seed(0)
    train_loader, test_loader, test_df, sizes, unpred, V = _loaders(bs=4)
    ds = train_loader.dataset
    ds.emo_labels = np.ones(len(ds.emo_labels), dtype=np.int64)
    opt = M.make_gan_opt(epochs=2, pair_bow_dim=V, best_model_path=str(tmp_path / "ckpt"), model_id="e2e_gan", vae_lr=1e-4)
    model = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=1300, layers=2), seed=1).to("cuda")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    optimizers = list(model.make_fused_optimizers(fuse_into_backward=True))
    assert len(optimizers) == 3
    logs = []
    best = T.train(train_loader, test_loader, model, optimizers, "cuda", num_unpred_pairs=unpred, opt=opt, log=logs.append)
    torch.cuda.synchronize()
    assert best is model
    after = model.state_dict()
    moved = {k for k in before if not torch.equal(before[k], after[k])}
    for k in R.GAN_KEYS + ("decoder.bias", "emotion_classifier.weight", "pair_classifier.weight", "encoder.encoder.layer.0.output.dense.weight",
                           "encoder.embeddings.word_embeddings.weight"):
        assert k in moved, k
    assert "emotion_mu.weight" not in moved and "cause_log_var.bias" not in moved       # in no optimiser group (:302-317)
    assert all(torch.isfinite(v).all() for v in after.values())
    assert sum("f1 socre" in str(l) for l in logs) == 2
    # train() writes a checkpoint only when an epoch's F1 beats the best so far (0 at the start): on the toy data an untrained pair head may
    # score F1 = 0 in both epochs, and then there is no file.  Saving and strict loading are checked unconditionally in
    # test_save_and_strict_load_round_trip; here the file, when written, must agree with the model train() returned
    ck = tmp_path / "ckpt" / "e2e_gan.pt"
    wrote = ck.exists()
    assert wrote == any("f1 socre: 0.0000" not in str(l) for l in logs if "f1 socre" in str(l)), logs
    if wrote:
        sd = torch.load(str(ck), map_location="cpu", weights_only=True)
        assert list(sd) == list(after)
        T.load_ckp(str(ck), M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=1300, layers=2), seed=2))
    df = T.generate_self_train_data(sizes, test_df, test_loader, model, "random")
    assert list(df.columns) == ["pair", "label", "emotion"] and set(df["label"]) <= {0, 1}
    preds = model.get_pair_preds(*(next(iter(test_loader))[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids")))
    assert len(preds) == len(test_df) and all(p[0] in (0.0, 1.0) for p in preds)
    # the same loop on stock torch optimisers over get_params()
    model2 = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=1300, layers=2), seed=1).to("cuda")
    opt.epochs, opt.model_id = 1, "e2e_gan_stock"
    b2 = {k: v.detach().clone() for k, v in model2.state_dict().items()}
    T.train(train_loader, test_loader, model2, stock_optimizers(model2, opt), "cuda", num_unpred_pairs=unpred, opt=opt, log=logs.append)
    a2 = model2.state_dict()
    assert all(not torch.equal(b2[k], a2[k]) for k in R.GAN_KEYS + ("decoder.weight",)) and all(torch.isfinite(v).all() for v in a2.values())


# ------------------------------------------------------------------------------------------------ (f) checkpoints
def test_save_and_strict_load_round_trip(golden_dir, tmp_path):
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    z, batch = load(golden_dir)
    wseed = int(z["meta"][5])
    model, P = build(opt, wseed)
    model.train()
    opts = model.make_fused_optimizers()
    model.set_noise(torch.from_numpy(z["eps_e_0"]), torch.from_numpy(z["eps_c_0"]))
    reference_step(model(*call(batch, 7)), opts)
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    sd = model.state_dict()
    assert [k for k in sd] == [str(k) for k in z["sd_keys"]]
    T.save_ckp(sd, str(tmp_path), "gan_rt")
    fresh = M.DrlClassifier(M.make_gan_opt(**vars(opt)), model.cfg, seed=5)
    T.load_ckp(os.path.join(str(tmp_path), "gan_rt.pt"), fresh)          # strict
    fresh.to("cuda")
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    assert not torch.equal(sd["ec_disc.weight"].cpu(), P["ec_disc.weight"]) and not torch.equal(sd["ce_disc.bias"].cpu(), P["ce_disc.bias"])
    # same weights, same noise, same seed: the loaded model computes the same step
    for m in (model, fresh):
        m.train()
        m._fwd_count = 100
        m.set_noise(torch.from_numpy(z["eps_e_1"]), torch.from_numpy(z["eps_c_1"]))
    a, b = model(*call(batch, 8)), fresh(*call(batch, 8))
    assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))
    # a checkpoint of the `none` model lacks the adversaries: strict load refuses it
    none_model, _ = build(opt, wseed, disentangle="none")
    with pytest.raises(RuntimeError, match="ec_disc"):
        M.DrlClassifier(M.make_gan_opt(**vars(opt)), model.cfg).load_state_dict(none_model.state_dict(), strict=True)
    with pytest.raises(L.CarelError):
        model.cpu()(*[v.cpu() if torch.is_tensor(v) else v for v in call(batch, 7)])
