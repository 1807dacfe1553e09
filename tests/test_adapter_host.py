"""CPU checks of the sentence-adapter feature (EMNLP scripts, drl_classifier_ec_mmd_final_mul_emnlp.py): the restated normalisers
the GPU tests use as their yardstick, and the model surface (state_dict keys and shapes, get_params, queries, argument checks)."""
import types

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from tests import adapter_restate as R


def _bisect(z, alpha):
    """float64 bisection for tau with sum max(z' - tau, 0)^(1/(alpha-1)) = 1 (z' = z for sparsemax, (z - max) / 2 for entmax15)."""
    z = z.double()
    x = z if alpha == 2 else (z - z.max(-1, keepdim=True).values) / 2
    power = 1.0 if alpha == 2 else 2.0
    lo = x.max(-1, keepdim=True).values - 1.0
    hi = x.max(-1, keepdim=True).values
    for _ in range(200):
        mid = (lo + hi) / 2
        f = torch.clamp(x - mid, min=0).pow(power).sum(-1, keepdim=True) - 1
        lo = torch.where(f > 0, mid, lo)
        hi = torch.where(f > 0, hi, mid)
    return torch.clamp(x - (lo + hi) / 2, min=0).pow(power)


def _rows():
    g = torch.Generator().manual_seed(3)
    rows = [torch.randn(16, 128, generator=g, dtype=torch.float64) * s for s in (0.3, 1.0, 4.0, 20.0)]
    tie = torch.zeros(4, 128, dtype=torch.float64)
    tie[:, :7] = 2.0                                  # an exact tie across the whole support
    tie[1, 7:9] = 1.0                                 # ties below it
    single = torch.full((2, 96), -5.0, dtype=torch.float64)
    single[:, 5] = 10.0                               # support of one
    const = torch.full((2, 32), 0.7, dtype=torch.float64)
    return rows + [tie, single, const]


@pytest.mark.parametrize("name", ["entmax", "sparsemax"])
def test_restated_normalisers_match_bisection_and_kkt(name):
    fn = R.entmax15 if name == "entmax" else R.sparsemax
    for z in _rows():
        p = fn(z)
        assert torch.allclose(p.sum(-1), torch.ones_like(p.sum(-1)), atol=1e-12)
        assert bool((p >= 0).all())
        ref = _bisect(z, 1.5 if name == "entmax" else 2)
        assert float((p - ref).abs().max()) < 1e-9
        # KKT: on the support the generalised gradient is constant; off it, it is below that constant
        x = (z - z.max(-1, keepdim=True).values) / 2 if name == "entmax" else z
        lhs = x - (p.sqrt() if name == "entmax" else p)       # = tau on the support
        sup = p > 0
        tau = torch.where(sup, lhs, torch.full_like(lhs, float("nan"))).nanmean(-1, keepdim=True)
        assert float(torch.where(sup, (lhs - tau).abs(), torch.zeros_like(lhs)).max()) < 1e-9
        assert bool((torch.where(sup, torch.full_like(x, -1e30), x) <= tau + 1e-12).all())
    const = R.entmax15(torch.full((1, 32), 0.7, dtype=torch.float64))
    assert torch.allclose(const, torch.full_like(const, 1 / 32))
    one = R.sparsemax(_rows()[5])
    assert bool((one[:, 5] == 1).all()) and int((one > 0).sum()) == 2


@pytest.mark.parametrize("name", ["entmax", "sparsemax"])
def test_restated_backward_matches_finite_differences(name):
    fn = R.entmax15_fn if name == "entmax" else R.sparsemax_fn
    g = torch.Generator().manual_seed(5)
    z = torch.randn(6, 64, generator=g, dtype=torch.float64) * 0.5
    p = (R.entmax15 if name == "entmax" else R.sparsemax)(z)
    assert int((p > 0).sum()) > 24                   # several elements per row on the support
    # every element at least 1e-3 away from the support boundary: the finite differences stay on one piece
    x = (z - z.max(-1, keepdim=True).values) / 2 if name == "entmax" else z
    tau = torch.stack([(x[i] - (p[i].sqrt() if name == "entmax" else p[i]))[p[i] > 0][0] for i in range(6)]).unsqueeze(1)
    assert float((x - tau).abs().min()) > 1e-3
    z = z.requires_grad_()
    assert torch.autograd.gradcheck(lambda t: fn(t, -1), (z,), eps=1e-7, atol=1e-6)


def _opt(**kw):
    return M.make_opt(pair_bow_dim=64, **kw)


def _model(**kw):
    return M.DrlClassifier(_opt(**kw), M.encoder_config("zh", vocab_size=100, layers=1), seed=7)


@pytest.mark.parametrize("mode,heads", [("entmax", 4), ("sparsemax", 4), ("raw", 4), ("raw", 12), ("entmax", 6)])
def test_adapter_state_dict_matches_the_reference_keys(mode, heads):
    base = set(_model().state_dict())
    m = _model(adapter=mode, head_number=heads)
    sd = m.state_dict()
    ref = R.reference_state_keys(mode, heads)
    want = {"%s_adapter.%s" % (side, k): v for side in ("emotion", "cause") for k, v in ref.items()}
    got = {k: tuple(v.shape) for k, v in sd.items() if k not in base}
    assert got == want
    assert set(sd) == base | set(want)
    # the reference registers the adapters between the encoder and the latent heads (:273-291)
    keys = list(sd)
    assert keys.index("emotion_adapter.in_proj_weight") < keys.index("emotion_mu.weight")
    # queries: buffers, not parameters, not in the state_dict; adapters are not optimised
    assert tuple(m.emotion_q.shape) == (1, 1, 768) and tuple(m.cause_q.shape) == (1, 1, 768)
    assert "emotion_q" not in sd and not any(k.endswith("_q") for k in dict(m.named_parameters()))
    ids = {id(p) for p in m.get_params()}
    for k, p in m.named_parameters():
        assert (id(p) in ids) == (k.split(".")[0] not in ("emotion_adapter", "cause_adapter", "emotion_mu", "emotion_log_var",
                                                         "cause_mu", "cause_log_var")), k
    # the adapters sit in the flat buffer beyond the optimised range
    assert all(m._offs[k] >= m._n_opt for k in m._adapter_names)
    # a reference-keyed checkpoint loads strictly
    src = {k: torch.randn(v) for k, v in want.items()}
    full = {k: v.clone() for k, v in sd.items()}
    full.update(src)
    m.load_state_dict(full, strict=True)
    for k, v in src.items():
        assert torch.equal(m.state_dict()[k], v)


def test_adapter_init_follows_the_reference_distributions():
    m = _model(adapter="sparsemax")
    a = m.emotion_adapter
    xav = (6.0 / (768 + 3 * 768)) ** 0.5
    assert float(a.in_proj_weight.detach().abs().max()) <= xav and float(a.in_proj_weight.detach().abs().max()) > 0.9 * xav
    assert float(a.in_proj_bias.detach().abs().max()) == 0.0 and float(a.out_proj.bias.detach().abs().max()) == 0.0
    lin = 1 / 768 ** 0.5
    for t in (a.out_proj.weight, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.v_proj.bias):
        t = t.detach()
        assert float(t.abs().max()) <= lin and float(t.abs().max()) > 0.9 * lin
    assert abs(float(m.emotion_q.std()) - 1.0) < 0.1 and not torch.equal(m.emotion_q, m.cause_q)
    # the seed generator draws them: same seed, same queries
    assert torch.equal(_model(adapter="sparsemax").emotion_q, m.emotion_q)


def test_no_adapter_is_todays_model():
    base = _model()
    for kw in (dict(adapter="false"), dict(adapter="false", head_number=5)):
        m = _model(**kw)
        assert list(m.state_dict()) == list(base.state_dict())
        assert m._order == base._order and m._n_opt == base._n_opt
        assert torch.equal(m._flat, base._flat)
        assert not hasattr(m, "emotion_q") and m._adapter_names == []
    legacy = types.SimpleNamespace(**{k: v for k, v in vars(_opt()).items()})
    assert not hasattr(legacy, "adapter")
    m = M.DrlClassifier(legacy, M.encoder_config("zh", vocab_size=100, layers=1), seed=7)
    assert torch.equal(m._flat, base._flat)


@pytest.mark.parametrize("kw", [dict(adapter="softmax"), dict(adapter="entmax", head_number=5), dict(adapter="raw", head_number=16),
                                dict(adapter="sparsemax", head_number=7), dict(adapter="entmax", disentangle="hsic"),
                                dict(adapter="raw", disentangle="vi")])
def test_bad_adapter_options_raise(kw):
    with pytest.raises(L.CarelError):
        _model(**kw)


@pytest.mark.parametrize("name", ["adapter_zh_entmax", "adapter_zh_sparsemax", "adapter_zh_raw", "adapter_en_entmax"])
def test_state_dict_equals_the_reference_models(golden_dir, name):
    """The key list and shapes recorded from the reference's own EMNLP DrlClassifier (tests/golden/gen_golden_adapter.py); a model built
    from that checkpoint's tensors loads them strictly and gives them back unchanged."""
    import os
    import numpy as np
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    B, S, Lr, vocab, V, wseed, bseed, steps, it0, heads, aseed = (int(v) for v in z["meta"])
    lang = "en" if str(z["variant"]) == "roberta" else "zh"
    cfg = M.encoder_config(lang, vocab_size=vocab, layers=Lr)
    m = M.DrlClassifier(M.make_opt(language=lang, pair_bow_dim=V, adapter=str(z["mode"]), head_number=heads), cfg, seed=1)
    sd = m.state_dict()
    want = {k: tuple(int(d) for d in s.split(",")) for k, s in zip(z["sd_keys"].tolist(), z["sd_shapes"].tolist())}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    ad = R.adapter_params(str(z["mode"]), heads, seed=aseed, kscale=float(z["kscale"]))
    assert set(ad) == {k for k in want if "_adapter." in k}
    m.load_state_dict({**{k: v.clone() for k, v in sd.items()}, **ad}, strict=True)
    for k, v in ad.items():
        assert torch.equal(m.state_dict()[k], v)


def test_the_english_adversarial_model_refuses_an_adapter():
    from carel_vae_amd import drl_classifier_en as E
    with pytest.raises(L.CarelError):
        E.DrlClassifier(E.make_opt(adapter="entmax", pair_bow_dim=64), E.encoder_config("en", vocab_size=100, layers=1))
