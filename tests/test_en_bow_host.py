"""Host-side checks of the zh three-space model and its element-weighted content losses (opt.language = "zh", opt.bow_loss):
the restatement tests/en_bow_restate.py against the fixtures tests/golden/gen_golden_zh3.py wrote from the reference's own
classes, the C ABI additions, and the option refusals.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from tests import en_bow_restate as R

CFG = O.EncoderConfig(layers=2, vocab_size=900)
OPT = OE.OptEn(pair_bow_dim=211, dropout=0.0, language="zh")
CASES = {"zh3_small": "plain", "zh3_bow_small": "bow"}


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    return z, {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}


def gslice(t, n=64):
    f = t.reshape(-1)
    step = max(1, f.numel() // n)
    return torch.cat((f[:n], f[-n:], f[::step][:n])).numpy()


def eps_of(z, s):
    return dict(con=torch.from_numpy(z[f"eps_con_{s}"]), e=torch.from_numpy(z[f"eps_e_{s}"]), c=torch.from_numpy(z[f"eps_c_{s}"]))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_the_reference_steps(golden_dir, name):
    """Losses at rtol 1e-5; gradient slices, norms, weights after three steps and get_pair_preds at the tolerances
    tests/test_oracle_golden.py uses for en_adv_small."""
    z, batch = load(golden_dir, name)
    B, S, Lr, vocab, V, wseed, bseed, steps = (int(v) for v in z["meta"])
    assert (B, S, Lr, vocab, V) == (16, 64, 2, 900, 211)
    P = OE.init_params(CFG, OPT, seed=wseed)
    states = [O.AdamState() for _ in range(6)]
    for s in range(steps):
        P, out, grads = R.train_step(P, batch, 7 + s, CFG, OPT, states, eps_of(z, s), weighting=CASES[name])
        got = np.array([float(out[n]) for n in R.LOSS_NAMES])
        np.testing.assert_allclose(got, z[f"losses_{s}"], rtol=1e-5, atol=0, err_msg=f"losses step {s}")
        if s == 1:
            for k in z.files:
                if k.startswith("g_"):
                    ref = z[k]
                    np.testing.assert_allclose(gslice(grads[k[2:]]), ref, rtol=2e-3, atol=2e-6 + 2e-4 * float(np.abs(ref).max()), err_msg=k)
                    np.testing.assert_allclose(float(grads[k[2:]].norm()), float(z["gn_" + k[2:]]), rtol=1e-3, atol=1e-7, err_msg=k)
    disc = tuple(g + "." for g in OE.DISC_GROUPS)
    for k in z.files:
        if k.startswith("w_"):
            lr = 10 * OPT.adv_lr if k[2:].startswith(disc) else OPT.vae_lr
            np.testing.assert_allclose(gslice(P[k[2:]]), z[k], atol=0.6 * lr, rtol=0, err_msg=k)
    logits = OE.pair_logits(P, batch["input_ids"], batch["attention_masks"], batch["token_type_ids"], CFG, OPT,
                            torch.from_numpy(z["pp_eps_e"]), torch.from_numpy(z["pp_eps_c"]))
    prob = torch.sigmoid(logits).numpy()
    assert z["pp_preds"].shape == (B, 1) and set(np.unique(z["pp_preds"])) <= {0.0, 1.0}
    clear = np.abs(prob - 0.5) > 1e-4
    np.testing.assert_array_equal(prob.round()[clear], z["pp_preds"][clear])


def test_the_two_fixtures_differ_where_the_weights_act(golden_dir):
    """The weighted script's content losses are about half the plain script's; what neither weights is the same number."""
    a, _ = load(golden_dir, "zh3_small")
    b, _ = load(golden_dir, "zh3_bow_small")
    assert np.array_equal(a["in_input_ids"], b["in_input_ids"]) and np.array_equal(a["eps_con_0"], b["eps_con_0"])
    la, lb = a["losses_0"], b["losses_0"]
    assert np.all(np.abs(lb[:2] - la[:2]) > 0.3 * la[:2])
    np.testing.assert_allclose(lb[2:6], la[2:6], rtol=1e-6)
    assert abs(lb[6] - la[6]) > 1e-3 * la[6]


def test_plain_weighting_is_the_oracle_tail():
    opt = OE.OptEn(pair_bow_dim=70, con_dim=8, ec_dim=4, dropout=0.5)
    cfg = O.EncoderConfig(layers=1, vocab_size=50)
    P = OE.init_params(cfg, opt, seed=3)
    g = torch.Generator().manual_seed(1)
    pooled = torch.randn(5, 768, generator=g)
    batch = OE.synthetic_batch(5, 16, cfg, 70, seed=2)
    eps = dict(con=torch.randn(8, generator=g), e=torch.randn(4, generator=g), c=torch.randn(4, generator=g))
    args = (P, pooled, batch["emo_labels"], batch["cau_labels"], batch["labels"], batch["bow_reps"], 11, opt, eps)
    want = OE.tail_forward(*args, train=True, seed=77)
    got = R.tail_forward(*args, weighting="plain", train=True, seed=77)
    for k in ("content_disc_emo", "content_disc_cau", "vae", "con_mul", "rec", "pair", "kl_con", "cent_e", "ent_ce"):
        np.testing.assert_allclose(float(got[k]), float(want[k]), rtol=1e-6, err_msg=k)
    bow = R.tail_forward(*args, weighting="bow", train=True, seed=77)
    assert float(bow["content_disc_emo"]) < 0.8 * float(want["content_disc_emo"]) and float(bow["rec"]) == float(got["rec"])
    m120 = O.dropout_scale_mask(77, R.SITE_CON_W, (5, 8), 0.5)
    m112 = O.dropout_scale_mask(77, OE.SITE_CMUL, (5, 8), 0.5)
    assert not torch.equal(m120, m112)


def test_abi_additions():
    from carel_vae_amd import _lib as L
    from carel_vae_amd import build
    lib = L.load()
    assert lib.carel_abi_version() == 9
    raw = ctypes.CDLL(build.lib_path())
    for n in ("carel_en_tail_bow_workspace_floats", "carel_en_tail_losses_bow"):
        assert hasattr(raw, n) and n in L.SIGNATURES and hasattr(lib, n)
    assert ctypes.sizeof(L.EnBowArgs) == ctypes.sizeof(ctypes.c_void_p)
    assert lib.carel_en_tail_workspace_floats(64, 24, 384, 23771) == 6489088      # unchanged by the weighted path
    n = lib.carel_en_tail_bow_workspace_floats(64, 384, 23771)
    assert n >= 64 * 384 + 64 * 23771 and n < 64 * 384 + 64 * 23771 + 256
    assert lib.carel_en_tail_bow_workspace_floats(1, 4, 1) > 0
    # refusals before any launch (no GPU is touched): null weight arguments / null scratch -> ARG (-1), oversize batch -> SHAPE (-2)
    a = L.EnTailArgs()
    assert lib.carel_en_tail_losses_bow(ctypes.byref(a), None, None) == -1
    b = L.EnBowArgs()
    a.hidden, a.batch, a.seq_len, a.ec_dim, a.con_dim, a.bow_dim = 768, 1025, 8, 24, 384, 211
    assert lib.carel_en_tail_losses_bow(ctypes.byref(a), ctypes.byref(b), None) == -2
    assert b"1..1024" in lib.carel_last_error()
    a.batch = 16
    keep = ctypes.create_string_buffer(64)
    for f in ("x_last_f32", "pooler_w", "pooler_b", "pooled", "lat"):
        setattr(a, f, ctypes.addressof(keep))
    for i in range(6):
        a.head_w[i] = a.head_b[i] = ctypes.addressof(keep)
    assert lib.carel_en_tail_losses_bow(ctypes.byref(a), ctypes.byref(b), None) == -1
    assert b"carel_en_tail_losses_bow: null weight scratch" in lib.carel_last_error()


def test_options_and_refusals():
    from carel_vae_amd import drl_classifier_en as ME
    from carel_vae_amd._lib import CarelError
    zh, bw, en = ME.make_zh_opt(), ME.make_bow_loss_opt(), ME.make_opt()
    assert (zh.language, zh.self_iteration, zh.bow_file) == ("zh", 30, "data/all_data_pair.txt") and not hasattr(zh, "bow_loss")
    assert (bw.language, bw.self_iteration, bw.bow_file, bw.bow_loss) == ("zh", 50, "data/all_data_pair.txt", True)
    assert en.language == "en" and en.self_iteration == 30
    assert ME.checkpoint_name(ME.make_zh_opt(model_id="x")) == "best_drl_model_x.pt"
    assert ME.checkpoint_name(ME.make_opt(model_id="x")) == "best_drl_en_model_x.pt"
    small = dict(pair_bow_dim=50, con_dim=8)
    tiny = lambda lang: ME.encoder_config(lang, vocab_size=100, layers=1)      # noqa: E731
    for v, want in ((False, False), ("false", False), (True, True), ("true", True)):
        m = ME.DrlClassifier(ME.make_zh_opt(bow_loss=v, **small), tiny("zh"))
        assert m.bow_loss is want and m.language == "zh"
    for bad in ("yes", 1, None, "True"):
        with pytest.raises(CarelError, match="bow_loss"):
            ME.DrlClassifier(ME.make_zh_opt(bow_loss=bad, **small), tiny("zh"))
    with pytest.raises(CarelError, match="bow_loss"):
        ME.DrlClassifier(ME.make_bow_loss_opt(adapter="entmax15", **small), tiny("zh"))
    with pytest.raises(CarelError, match="adapter"):
        ME.DrlClassifier(ME.make_zh_opt(adapter="entmax15", **small), tiny("zh"))
    with pytest.raises(CarelError, match="language"):
        ME.DrlClassifier(ME.make_opt(language="fr", **small), tiny("en"))
    # opt.language picks the encoder geometry when no config is given; the variant adds no parameter
    plain = ME.DrlClassifier(ME.make_zh_opt(**small), tiny("zh"))
    weighted = ME.DrlClassifier(ME.make_bow_loss_opt(**small), tiny("zh"))
    assert list(plain.state_dict()) == list(weighted.state_dict())
    assert plain.cfg.type_vocab == 2 and plain.state_dict()["encoder.embeddings.token_type_embeddings.weight"].shape[0] == 2
    full = ME.encoder_config("zh")
    assert (full.vocab_size, full.type_vocab, full.ln_eps, full.roberta) == (21128, 2, 1e-12, 0)


def test_zh_reader_contract(golden_dir):
    from carel_vae_amd import data as D
    from carel_vae_amd import drl_classifier_en as ME
    import random
    path = os.path.join(golden_dir, "ecpe", "sample_zh_test.txt")
    got = ME.read_ECPE_data(path, test=True, language="zh", rng=random.Random(1))
    want = D.read_ECPE_data(path, test=True, language="zh", rng=random.Random(1))
    assert len(got) == 3 and got[0].equals(want[0]) and got[1] == want[1] and got[2] == want[2]
