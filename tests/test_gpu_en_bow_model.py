"""The zh three-space model (opt.language = "zh", drl_classifier.py) and its element-weighted variant (opt.bow_loss,
drl_classifier_bow_loss.py) on the HIP path, against (a) the fixtures tests/golden/gen_golden_zh3.py wrote from the reference's own
classes (fp32 CPU) and (b) the restatement tests/en_bow_restate.py with bf16 rounding at the encoder kernels' storage points.
Tolerances are those of tests/test_gpu_en_adv.py."""
import os

import numpy as np
import pytest
import torch

from carel_vae_amd import drl_classifier as M
from carel_vae_amd import drl_classifier_en as ME
from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from tests import en_bow_restate as R

pytestmark = pytest.mark.gpu

CFG = O.EncoderConfig(layers=2, vocab_size=900)
DISC = tuple(g + "." for g in OE.DISC_GROUPS)
CASES = [("zh3_small", False), ("zh3_bow_small", True)]
TERM_MAP = dict(zip(ME.TERM_NAMES, OE.LOSS_NAMES + ("cent_e", "cent_c", "ent_ed", "ent_cad", "ent_ec", "ent_ce", "emo_mul", "cau_mul", "con_mul",
                                                  "pair", "kl_e", "kl_c", "kl_con", "rec")))


def build(opt, wseed, bow_loss, train_dropout=False, cfg=CFG):
    mcfg = M.encoder_config("zh", vocab_size=cfg.vocab_size, layers=cfg.layers, hidden_dropout=cfg.hidden_dropout if train_dropout else 0.0,
                            attn_dropout=cfg.attn_dropout if train_dropout else 0.0)
    kw = {k: v for k, v in vars(opt).items() if k in ME.DEFAULT_OPT}
    model = ME.DrlClassifier(ME.make_bow_loss_opt(**kw) if bow_loss else ME.make_zh_opt(**kw), mcfg)
    P = OE.init_params(cfg, opt, seed=wseed)
    model.load_state_dict(P)
    model.to("cuda")
    return model, P


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    return z, {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}


def call(batch, it):
    b = {k: v.cuda() for k, v in batch.items()}
    return (b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], it)


def eps_of(z, s):
    return dict(con=torch.from_numpy(z[f"eps_con_{s}"]), e=torch.from_numpy(z[f"eps_e_{s}"]), c=torch.from_numpy(z[f"eps_c_{s}"]))


def relnorm(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def gslice(t, n=64):
    f = t.detach().cpu().reshape(-1)
    step = max(1, f.numel() // n)
    return torch.cat((f[:n], f[-n:], f[::step][:n])).numpy()


def reference_step(losses, opts):
    """The backward / zero_grad sequence of the reference's loop (drl_classifier.py:843-863)."""
    cd_e, cd_c, ed, ecd, cad, ced, vae = losses
    opts[0].zero_grad(); (cd_e + cd_c).backward(retain_graph=True)        # noqa: E702
    opts[1].zero_grad(); ed.backward(retain_graph=True)                  # noqa: E702
    opts[3].zero_grad(); ecd.backward(retain_graph=True)                 # noqa: E702
    opts[2].zero_grad(); cad.backward(retain_graph=True)                 # noqa: E702
    opts[4].zero_grad(); ced.backward(retain_graph=True)                 # noqa: E702
    opts[5].zero_grad(); vae.backward()                                  # noqa: E702


def torch_opts(model, opt):
    gp = model.get_params()
    return [torch.optim.RMSprop(g, lr=opt.adv_lr) for g in gp[:5]] + [torch.optim.Adam(gp[5], lr=opt.vae_lr)]


@pytest.mark.parametrize("name,bow_loss", CASES)
def test_terms_and_gradients_vs_restatement_and_golden(golden_dir, name, bow_loss):
    opt = OE.OptEn(pair_bow_dim=211, dropout=0.0, language="zh")
    z, batch = load(golden_dir, name)
    wseed = int(z["meta"][5])
    model, P = build(opt, wseed, bow_loss)
    assert model.bow_loss is bow_loss and model.language == "zh" and model.cfg.type_vocab == 2
    model.train()
    # step 0: the seven losses against the golden, every term against the restatement
    eps = eps_of(z, 0)
    model.set_noise(eps["con"], eps["e"], eps["c"])
    losses = model(*call(batch, 7))
    got = np.array([float(v.detach()) for v in losses])
    print(name, "step 0 losses", got, "golden", z["losses_0"])
    np.testing.assert_allclose(got, z["losses_0"], rtol=2e-2, atol=1e-3)
    weighting = "bow" if bow_loss else "plain"
    ref = R.forward_terms(P, batch, 7, CFG, opt, eps, weighting=weighting, quant=O.bf16_round)
    terms = {k: float(v) for k, v in model.last_terms().items()}
    for mine, theirs in TERM_MAP.items():
        r = float(ref[theirs])
        assert abs(terms[mine] - r) <= 3e-3 * max(abs(r), 1e-3) + 1e-6, (mine, terms[mine], r)
    assert relnorm(model._last_call.buf.z, ref["z"]) < 1e-2
    # the gradients every optimiser sees, as tests/test_gpu_en_adv.py checks them
    ref, grads = R.loss_and_grads(P, batch, 7, CFG, opt, eps, weighting=weighting, quant=O.bf16_round)
    reference_step(losses, torch_opts(model, opt))
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    worst = {}
    for k, g in grads.items():
        got = named[k].grad
        assert got is not None, k
        if float(g.norm()) < 1e-7 or k.endswith("key.bias"):
            continue
        if g.numel() == 1:
            assert abs(float(got) - float(g)) <= 4e-2 * abs(float(g)) + 2e-2, (k, float(got), float(g))
            continue
        worst[k] = relnorm(got, g)
    bad = {k: v for k, v in worst.items() if v > (1.5e-2 if not k.startswith("encoder.") else 4e-2)}
    assert not bad, bad
    for h in OE.LATENT_HEADS:
        assert named[h + ".weight"].grad is None


@pytest.mark.parametrize("name,bow_loss", CASES)
def test_three_steps_follow_the_reference(golden_dir, name, bow_loss):
    """Losses of every step, the gradient slices of step 1 and the weights after three steps of the reference's order."""
    opt = OE.OptEn(pair_bow_dim=211, dropout=0.0, language="zh")
    z, batch = load(golden_dir, name)
    B, S, Lr, vocab, V, wseed, bseed, steps = (int(v) for v in z["meta"])
    model, P = build(opt, wseed, bow_loss)
    model.train()
    opts = torch_opts(model, opt)
    named = dict(model.named_parameters())
    for s in range(steps):
        eps = eps_of(z, s)
        model.set_noise(eps["con"], eps["e"], eps["c"])
        losses = model(*call(batch, 7 + s))
        reference_step(losses, opts)
        if s == 1:
            for k in z.files:
                if k.startswith("g_") and not k.endswith("key.bias") and float(z["gn_" + k[2:]]) > 1e-7 and z[k].size > 3:
                    tol = 1.5e-2 if not k[2:].startswith("encoder.") else 4e-2
                    assert abs(float(named[k[2:]].grad.norm()) - float(z["gn_" + k[2:]])) <= tol * float(z["gn_" + k[2:]]), k
        for o in opts:
            o.step()
        got = np.array([float(v.detach()) for v in losses])
        np.testing.assert_allclose(got, z[f"losses_{s}"], rtol=2e-2, atol=2e-3, err_msg=f"step {s}")
    sd = model.state_dict()
    for k in z.files:
        if k.startswith("w_"):
            pk = k[2:]
            lr = 10 * opt.adv_lr if pk.startswith(DISC) else opt.vae_lr
            d = np.abs(gslice(sd[pk]) - z[k])
            assert d.max() <= 2 * steps * lr * 1.01, pk
            if not pk.endswith("key.bias"):
                assert (d <= 1.2 * lr).mean() >= 0.95, (pk, float((d <= 1.2 * lr).mean()))


def test_the_weighted_fixture_needs_the_weighted_path(golden_dir):
    """zh3_bow_small loaded into a model built WITHOUT bow_loss misses content_disc_loss_emo by more than 30 %: the fixture tells the
    feature from an option that is silently ignored."""
    opt = OE.OptEn(pair_bow_dim=211, dropout=0.0, language="zh")
    z, batch = load(golden_dir, "zh3_bow_small")
    model, _ = build(opt, int(z["meta"][5]), bow_loss=False)
    model.train()
    eps = eps_of(z, 0)
    model.set_noise(eps["con"], eps["e"], eps["c"])
    with torch.no_grad():
        losses = model(*call(batch, 7))
    want = float(z["losses_0"][0])
    assert abs(float(losses[0]) - want) > 0.3 * want, (float(losses[0]), want)
    np.testing.assert_allclose(float(losses[2]), z["losses_0"][2], rtol=2e-2)        # what the variant does not touch still agrees


@pytest.mark.parametrize("name,bow_loss", CASES)
def test_get_pair_preds_returns_the_rounded_list(golden_dir, name, bow_loss):
    opt = OE.OptEn(pair_bow_dim=211, dropout=0.0, language="zh")
    z, batch = load(golden_dir, name)
    model, P = build(opt, int(z["meta"][5]), bow_loss)
    # the golden's predictions come from the weights AFTER its three steps: rebuild those with the restatement
    states = [O.AdamState() for _ in range(6)]
    for s in range(int(z["meta"][7])):
        P, _, _ = R.train_step(P, batch, 7 + s, CFG, opt, states, eps_of(z, s), weighting="bow" if bow_loss else "plain")
    model.load_state_dict(P)
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    noise = (torch.zeros(opt.con_dim), torch.from_numpy(z["pp_eps_e"]), torch.from_numpy(z["pp_eps_c"]))
    model.set_noise(*noise)
    got = model.get_pair_preds(b["input_ids"], b["attention_masks"], b["token_type_ids"])
    assert isinstance(got, list) and len(got) == len(batch["input_ids"]) and isinstance(got[0], list) and isinstance(got[0][0], float)
    assert set(v[0] for v in got) <= {0.0, 1.0}
    model.set_noise(*noise)
    prob = np.array(model.get_pair_preds(b["input_ids"], b["attention_masks"], b["token_type_ids"], round=False))
    assert prob.shape == (len(got), 1) and np.array_equal(prob.round(), np.array(got))
    # bf16 encoder here, fp32 in the reference: a probability within 5e-3 of one half may round the other way
    clear = np.abs(prob - 0.5) > 5e-3
    assert clear.sum() >= len(got) - 2
    np.testing.assert_array_equal(np.array(got)[clear], z["pp_preds"][clear])


def test_site_120_dropout_statistics():
    """Dropout ON (p = 0.5): the keep-rate of the weight input's own copy (site 120) within the bound tests/test_gpu_gemm.py uses for its
    dropout statistics, its mask different from site 112's on the same elements, and both equal to the restatement's counter-based masks."""
    opt = OE.OptEn(pair_bow_dim=211, dropout=0.5, language="zh")
    cfg = O.EncoderConfig(layers=1, vocab_size=300)
    model, P = build(opt, 7, bow_loss=True, train_dropout=True, cfg=cfg)
    model.train()
    B = 64
    batch = OE.synthetic_batch(B, 32, cfg, 211, seed=4, shape="B")
    g = torch.Generator().manual_seed(2)
    eps = dict(con=torch.randn(opt.con_dim, generator=g), e=torch.randn(opt.ec_dim, generator=g), c=torch.randn(opt.ec_dim, generator=g))
    model.set_noise(eps["con"], eps["e"], eps["c"])
    losses = model(*call(batch, 9))
    c = model._last_call
    Cd, Dd = opt.con_dim, opt.ec_dim
    z_con = c.buf.z[:, 2 * Dd:].cpu()
    x120 = c.buf.bow_work[:B * Cd].reshape(B, Cd).cpu()
    m120 = (x120 != 0)
    assert abs(float(m120.float().mean()) - 0.5) < 0.01
    want120 = O.dropout_scale_mask(c.seed, R.SITE_CON_W, (B, Cd), 0.5)
    want112 = O.dropout_scale_mask(c.seed, OE.SITE_CMUL, (B, Cd), 0.5)
    assert torch.equal(x120, z_con * want120)
    assert float(((want120 != 0) != (want112 != 0)).float().mean()) > 0.4          # independent masks disagree on about half the elements
    ref = R.forward_terms(P, batch, 9, cfg, opt, eps, weighting="bow", train=True, seed=c.seed, quant=O.bf16_round)
    got = np.array([float(v.detach()) for v in losses])
    want = np.array([float(ref[n]) for n in R.LOSS_NAMES])
    np.testing.assert_allclose(got, want, rtol=4e-3, atol=1e-5)
