"""opt.disentangle == "gan" (drl_classifier_ec_gan.py) without a GPU: the restatement the GPU tests measure against is itself checked
against the reference class (fixture gan_small.npz, written by tests/golden/gen_golden_gan.py), and the host side of the option --
state_dict keys, optimiser groups, flat ranges, defaults, refusals, argument validation of carel_gan_disc -- is checked here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from oracle import carel_oracle as O
from tests import gan_restate as R

CFG = O.EncoderConfig(layers=2, vocab_size=900)


def load(golden_dir, name="gan_small"):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, batch


def gslice(t, n=64):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return torch.cat((f[:n], f[-n:], f[::step][:n])).numpy()


def small_model(**kw):
    return M.DrlClassifier(M.make_gan_opt(pair_bow_dim=211, **kw), M.encoder_config("zh", vocab_size=CFG.vocab_size, layers=CFG.layers))


def test_restatement_follows_the_reference_class(golden_dir):
    """Three steps of the script's loop (two RMSprop adversaries + Adam): the three losses, the gradient every optimiser sees at step 1,
    the weights after the last step and get_pair_preds.  Bounds: those tests/test_oracle_golden.py uses for its fp32 restatement of the
    three-space adversarial script (test_en_adversarial_three_space_steps)."""
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    z, batch = load(golden_dir)
    B, S, Lr, vocab, V, wseed, bseed, steps = (int(v) for v in z["meta"])
    P = R.init_params(CFG, opt, wseed)
    states = [O.AdamState() for _ in range(3)]
    for s in range(steps):
        eps_e, eps_c = torch.from_numpy(z[f"eps_e_{s}"]), torch.from_numpy(z[f"eps_c_{s}"])
        P, out, grads = R.train_step(P, batch, 7 + s, CFG, opt, states, eps_e, eps_c)
        got = np.array([float(out[n]) for n in R.LOSS_NAMES])
        np.testing.assert_allclose(got, z[f"losses_{s}"], rtol=3e-5, atol=2e-6, err_msg=f"losses step {s}")
        if s == 1:
            seen = 0
            for k in z.files:
                if k.startswith("g_"):
                    ref = z[k]
                    np.testing.assert_allclose(gslice(grads[k[2:]]), ref, rtol=2e-3, atol=2e-6 + 2e-4 * float(np.abs(ref).max()), err_msg=k)
                    np.testing.assert_allclose(float(grads[k[2:]].norm()), float(z["gn_" + k[2:]]), rtol=1e-3, atol=1e-7, err_msg=k)
                    seen += 1
            assert seen > 20 and all("g_" + k in z.files for k in R.GAN_KEYS)
    for k in z.files:
        if k.startswith("w_"):
            lr = 10 * opt.adv_lr if k[2:] in R.GAN_KEYS else opt.vae_lr      # an RMSprop step is up to lr / sqrt(1 - alpha)
            np.testing.assert_allclose(gslice(P[k[2:]]), z[k], atol=0.6 * lr, rtol=0, err_msg=k)
    prob = O.pair_preds(P, batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], CFG, R.oracle_opt(opt),
                        torch.from_numpy(z["pp_eps_e"]), torch.from_numpy(z["pp_eps_c"]))
    clear = (prob - 0.5).abs().reshape(-1) > 1e-4           # a probability that close to 1/2 may round either way
    assert clear.sum() >= B - 1
    assert np.array_equal(prob.round().numpy().reshape(-1)[clear.numpy()], z["pp_preds"].reshape(-1)[clear.numpy()])


def test_the_detached_adversaries_leave_every_other_gradient_alone(golden_dir):
    """What the two .detach() calls imply (the GPU test pins it bit for bit on the kernels): the gradient of every non-discriminator tensor under
    the vae loss equals that of the `none` model with the BCE head; the entropy terms reach the discriminators only."""
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
    z, batch = load(golden_dir)
    wseed = int(z["meta"][5])
    P = R.init_params(CFG, opt, wseed)
    eps_e, eps_c = torch.from_numpy(z["eps_e_0"]), torch.from_numpy(z["eps_c_0"])
    out, grads = R.loss_and_grads(P, batch, 7, CFG, opt, eps_e, eps_c)
    Pn = {k: v for k, v in P.items() if k not in R.GAN_KEYS}
    ref, gn = O.loss_and_grads(Pn, batch, 7, CFG, R.oracle_opt(opt), eps_e, eps_c, disentangle="none", emotion_head="bce")
    # the same fp32 sums in both graphs; only autograd's order of accumulation may differ (the embedding scatter is not
    # deterministic on the CPU): a few units of fp32 rounding (6e-8) on the norm
    for k in O.optimised_keys(CFG, R.oracle_opt(opt)):
        assert float((gn[k] - grads[k]).norm()) <= 1e-6 * float(gn[k].norm()), k
    want = float(ref["loss"]) + opt.ecce_adv_loss_weight * (float(out["ec_entropy"]) + float(out["ce_entropy"]))
    assert abs(float(out["vae"]) - want) <= 1e-6 * abs(want)


def test_state_dict_keys_and_shapes_are_the_reference_scripts(golden_dir):
    z, _ = load(golden_dir)
    model = small_model()
    sd = model.state_dict()
    want = [str(k) for k in z["sd_keys"]]
    assert list(sd) == want                                     # same names, same order: ec_disc / ce_disc between cause_log_var and emotion_classifier
    assert [list(sd[k].shape) for k in want] == json.loads(str(z["sd_shapes"]))
    assert want == R.state_dict_keys(CFG, R.gan_opt(pair_bow_dim=211))
    i = want.index("ec_disc.weight")
    assert want[i - 1] == "cause_log_var.bias" and want[i:i + 5] == list(R.GAN_KEYS) + ["emotion_classifier.weight"]
    # a state_dict with the script's keys loads strictly
    model.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    with pytest.raises(RuntimeError):
        M.DrlClassifier(M.make_opt(pair_bow_dim=211, e_num_class=1, disentangle="none", emotion_head="bce"),
                        M.encoder_config("zh", vocab_size=CFG.vocab_size, layers=CFG.layers)).load_state_dict(sd, strict=True)


def test_optimiser_groups_and_flat_ranges(golden_dir):
    z, _ = load(golden_dir)
    model = small_model()
    groups = model.get_params()
    assert isinstance(groups, tuple) and len(groups) == 3
    names = {id(p): k for k, p in model.named_parameters()}
    got = [[names[id(p)] for p in g] for g in groups]
    want = json.loads(str(z["group_keys"]))
    assert got[0] == want[0] == ["ec_disc.weight", "ec_disc.bias"] and got[1] == want[1] == ["ce_disc.weight", "ce_disc.bias"]
    heads = lambda ks: [k for k in ks if not k.startswith("encoder.")]     # noqa: E731   (encoder keys: HF's own order, compared as a set)
    assert heads(got[2]) == heads(want[2]) and set(got[2]) == set(want[2])
    assert not any(k.startswith(("emotion_mu", "emotion_log_var", "cause_mu", "cause_log_var")) for g in got for k in g)
    # flat buffer: [vae group | ec_disc | ce_disc | latent heads], every group one aligned contiguous range
    r, offs = model._group_ranges, model._offs
    assert r["vae"] == (0, model._n_opt) and r["vae"][1] == r["ec_disc"][0] and r["ec_disc"][1] == r["ce_disc"][0]
    assert r["ce_disc"][1] == offs["emotion_mu.weight"]
    for g in ("ec_disc", "ce_disc"):
        lo, hi = r[g]
        assert lo % 64 == 0 and hi % 64 == 0 and lo <= offs[g + ".weight"] < offs[g + ".bias"] < hi
    for k in got[2]:
        assert offs[k] + model._named[k].numel() <= r["vae"][1], k
    for k, p in model.named_parameters():                     # every parameter is a view of the flat buffer
        assert p.data_ptr() == model._flat.data_ptr() + 4 * offs[k]


def test_make_gan_opt_carries_the_scripts_defaults(golden_dir):
    z, _ = load(golden_dir)
    rec = json.loads(str(z["defaults"]))
    opt = M.make_gan_opt()
    for k, v in rec.items():
        assert getattr(opt, k) == v, k
    assert rec["pair_mul_loss_weight"] == 25 and rec["adv_lr"] == 0.003 and rec["ecce_adv_loss_weight"] == 1 and rec["epochs"] == 10
    assert opt.disentangle == "gan" and opt.emotion_head == "bce" and opt.e_num_class == opt.c_num_class == opt.pair_num_class == 1
    assert vars(R.gan_opt()) == {k: getattr(opt, k) for k in vars(R.gan_opt())}
    assert M.make_gan_opt(ec_dim=32).ec_dim == 32


def test_refusals_name_their_reason():
    with pytest.raises(L.CarelError, match="emotion_head"):
        small_model(emotion_head="ce")
    for name in ("e_num_class", "c_num_class", "pair_num_class", "ec_num_class"):
        with pytest.raises(L.CarelError, match="num_class"):
            small_model(**{name: 2})
    with pytest.raises(L.CarelError, match="adapter"):
        small_model(adapter="entmax")
    from carel_vae_amd import dp
    with pytest.raises(L.CarelError, match="DataParallel"):
        dp.DataParallel(small_model())
    with pytest.raises(L.CarelError, match="gan"):                 # the fused triple belongs to the option
        M.DrlClassifier(M.make_opt(pair_bow_dim=211), M.encoder_config("zh", vocab_size=100, layers=1)).make_fused_optimizers()
    model = small_model()
    zi = torch.zeros((2, 128), dtype=torch.long)
    with pytest.raises(L.CarelError):                              # no CPU fallback
        model(zi, zi, zi, torch.ones(2, 1), torch.zeros(2, 1), torch.zeros(2, 1), torch.zeros(2, 211), 0)


def test_carel_gan_disc_validates_before_any_hip_call():
    lib = L.load()
    assert lib.carel_abi_version() == 9                            # additive change: a new function and a new struct
    assert lib.carel_gan_disc(None, None) == -1
    assert b"carel_gan_disc" in lib.carel_last_error() and b"null" in lib.carel_last_error()
    a = L.GanArgs()
    assert lib.carel_gan_disc(ctypes.byref(a), None) == -1          # null tensors
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def filled(batch, ec_dim):
        a = L.GanArgs()
        a.z = a.emo_labels = a.cau_labels = a.terms = p
        for i in range(2):
            a.disc_w[i] = a.disc_b[i] = a.g_loss_w[i] = a.g_loss_b[i] = a.g_ent_w[i] = a.g_ent_b[i] = p
        a.batch, a.ec_dim, a.label_smoothing, a.epsilon = batch, ec_dim, 0.1, 1e-8
        return a
    for batch, ec_dim in ((0, 24), (1025, 24), (16, 0), (16, 33), (-3, 24)):
        assert lib.carel_gan_disc(ctypes.byref(filled(batch, ec_dim)), None) == -2, (batch, ec_dim)
        msg = lib.carel_last_error()
        assert b"carel_gan_disc" in msg and b"batch" in msg and b"ec_dim" in msg
    a = filled(16, 24)
    a.g_ent_b[1] = None
    assert lib.carel_gan_disc(ctypes.byref(a), None) == -1 and b"discriminator" in lib.carel_last_error()
    a = filled(16, 24)
    a.drop_p = 1.5
    assert lib.carel_gan_disc(ctypes.byref(a), None) == -1 and b"drop_p" in lib.carel_last_error()
