"""The paths that produce the reported numbers -- DrlClassifier.pair_latents / pair_probabilities / get_pair_preds and the three-space
pair_logits / get_pair_preds -- against the CPU oracle ROW BY ROW (a whole-tensor norm lets one bad row among 300 through at a few
percent), and against themselves bitwise: a row of the result depends on its own sentence only, whatever chunk it travels in.

Cases, parameters, oracle outputs and tolerances come from tests/eval_restate.py (TOL_ROW_LATENT, TOL_PROB: three times the measured gap
between the fp32 oracle and the bf16_round oracle; tests/test_eval_restate_host.py holds them to that).  Two encoder layers, S of 32 or
64, a vocabulary of 300; every model and oracle output is built once per process.  `pytest -s` prints the worst fraction of each tolerance.

The exact properties (slice, neighbours, padding content, length rounding) are asserted with torch.equal: launch shapes and each row's
arithmetic are the same on both sides."""
import numpy as np
import pytest
import torch

from carel_vae_amd import drl_classifier as M
from carel_vae_amd import drl_classifier_en as ME
from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from tests import eval_restate as R
from tests.gpu_util import bits, rel_err

pytestmark = pytest.mark.gpu
_models, _gpu = {}, {}


def model_of(name):
    if name not in _models:
        cfg, opt, _ = R.MODELS[name]
        mcfg = M.encoder_config("en" if cfg.variant == "roberta" else "zh", vocab_size=cfg.vocab_size, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab,
                                ln_eps=cfg.ln_eps, layers=cfg.layers, hidden_dropout=0.0, attn_dropout=0.0)
        m = M.DrlClassifier(M.make_opt(**vars(opt)), mcfg)
        m.load_state_dict(R.params(name))                       # init_params, pair head calibrated on the oracle
        _models[name] = m.to("cuda").eval()
    return _models[name]


def gpu_batch(case):
    if case not in _gpu:
        b = R.case_batch(case)
        _gpu[case] = tuple(b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
    return _gpu[case]


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check_rows(lat, case, what=""):
    """every row of lat within TOL_ROW_LATENT of the fp32 oracle and of the bf16_round oracle; returns the two worst fractions"""
    out = []
    for emu in (False, True):
        rel = R.row_rel(lat, R.oracle_latents(case, emu))
        assert float(rel.max()) <= R.TOL_ROW_LATENT, (case, what, "bf16_round" if emu else "fp32", int(rel.argmax()), float(rel.max()))
        out.append(float(rel.max()) / R.TOL_ROW_LATENT)
    return out


# ------------------------------------------------------------------------------------------------ A.1 latents per row
@pytest.mark.parametrize("case", list(R.EVAL_CASES))
def test_pair_latents_rows_against_the_oracle_at_every_chunk(case):
    name, N, S, kind = R.EVAL_CASES[case]
    m, b = model_of(name), gpu_batch(case)
    for chunk in R.chunks_of(N):
        lat = m.pair_latents(*b, chunk=chunk)
        assert lat.shape == (N, 4 * R.MODELS[name][1].ec_dim) and lat.dtype == torch.float32
        f = check_rows(lat, case, chunk)
        print("\npair_latents %s chunk=%d: worst row %.3f (fp32) %.3f (bf16_round) of TOL_ROW_LATENT" % (case, chunk, f[0], f[1]))
    if kind == "lastfull":                  # the last chunk has no padding and runs dense, the chunks before it run packed
        c0 = m._prepare_inputs(b[0][:8], b[1][:8], b[2][:8])
        c1 = m._prepare_inputs(b[0][128:], b[1][128:], b[2][128:])
        assert c0.pack is not None and c1.pack is None


# ------------------------------------------------------------------------------------------------ A.2 probabilities
@pytest.mark.parametrize("case", list(R.EVAL_CASES))
def test_probabilities_and_predictions_against_the_oracle(case):
    name, N, S, kind = R.EVAL_CASES[case]
    m, b = model_of(name), gpu_batch(case)
    eps_e, eps_c = R.noise(name)
    want = R.oracle_prob(case)              # float64 sigmoid of the fp32 oracle's latents under the same noise
    for chunk in R.chunks_of(N):
        m.set_noise(eps_e, eps_c)
        p = m.pair_probabilities(*b, chunk=chunk)
        d = float((p.double().cpu() - want).abs().max())
        assert p.shape == (N,) and d <= R.TOL_PROB, (case, chunk, d)
    m.set_noise(eps_e, eps_c)
    raw = m.get_pair_preds(*b, round=False)
    assert isinstance(raw, list) and len(raw) == N and all(isinstance(r, list) and len(r) == 1 for r in raw)
    d2 = float((torch.tensor(raw, dtype=torch.float64).reshape(-1) - want).abs().max())
    assert d2 <= R.TOL_PROB, (case, d2)
    print("\nprobabilities %s: %.3f (chunked) %.3f (get_pair_preds) of TOL_PROB" % (case, d / R.TOL_PROB, d2 / R.TOL_PROB))
    m.set_noise(eps_e, eps_c)
    preds = torch.tensor(m.get_pair_preds(*b), dtype=torch.float64).reshape(-1)
    far = (want - 0.5).abs() > R.FAR
    assert torch.equal(preds[far], want.round()[far])
    if N > 1:
        assert set(preds[far].tolist()) == {0.0, 1.0}            # both classes occur among the compared rows


# ------------------------------------------------------------------------------------------------ A.3 exact properties
@pytest.mark.parametrize("case,chunk", [("zh24_B_300", 128), ("zh24_B_300", 8), ("zh24_B_5", 1), ("zh24_lastfull", 8), ("en24_B_129", 8), ("zh32_B_129", 128)])
def test_slice_property_bitwise(case, chunk):
    """rows [s, s + c) of pair_latents(all, chunk=c) are pair_latents of that slice alone"""
    name, N = R.EVAL_CASES[case][:2]
    m, b = model_of(name), gpu_batch(case)
    full = m.pair_latents(*b, chunk=chunk).clone()
    for s in range(0, N, chunk):
        alone = m.pair_latents(*(t[s:s + chunk] for t in b), chunk=chunk)
        assert same_bits(full[s:s + chunk], alone), (case, chunk, s)


@pytest.mark.parametrize("case", ["zh24_B_129", "zh24_mix", "en24_B_129"])
def test_neighbour_property_bitwise(case):
    """every second sample replaced by a different sentence of the same length: the untouched samples' rows keep their bits"""
    name, N = R.EVAL_CASES[case][:2]
    cfg = R.MODELS[name][0]
    m, b = model_of(name), gpu_batch(case)
    ids = b[0].clone()
    rs = np.random.RandomState(5)
    lens = R.case_lengths(case)
    for i in range(1, N, 2):
        ids[i, :lens[i]] = torch.from_numpy(rs.randint(2, cfg.vocab_size, size=lens[i])).cuda()
    for chunk in (N, 8):
        base = m.pair_latents(*b, chunk=chunk).clone()
        got = m.pair_latents(ids, b[1], b[2], chunk=chunk)
        assert same_bits(got[0::2], base[0::2]), (case, chunk)
        assert not torch.equal(got[1::2], base[1::2])


@pytest.mark.parametrize("varlen", [True, False])
@pytest.mark.parametrize("case", ["zh24_B_129", "zh24_mix", "en24_B_129"])
def test_padding_content_does_not_matter_bitwise(case, varlen):
    """ids and token types under mask 0 overwritten with random valid ids: nothing changes, packed or dense"""
    name, N = R.EVAL_CASES[case][:2]
    cfg = R.MODELS[name][0]
    m, b = model_of(name), gpu_batch(case)
    g = torch.Generator().manual_seed(3)
    pad = b[1] == 0
    ids = torch.where(pad, torch.randint(0, cfg.vocab_size, b[0].shape, generator=g).cuda(), b[0])
    tt = torch.where(pad, torch.randint(0, cfg.type_vocab, b[2].shape, generator=g).cuda(), b[2])
    assert not torch.equal(ids, b[0])
    m.varlen = varlen
    try:
        for chunk in (N, 8):
            base = m.pair_latents(*b, chunk=chunk).clone()
            assert same_bits(m.pair_latents(ids, b[1], tt, chunk=chunk), base), (case, varlen, chunk)
    finally:
        m.varlen = True


@pytest.mark.parametrize("name", ["zh24", "en24"])
def test_length_rounding_bitwise(name):
    """an input of 40 positions is the same input padded by hand to 64 with masked positions"""
    cfg = R.MODELS[name][0]
    m = model_of(name)
    lens = [40, 2, 33, 17, 39, 40, 8]
    b = R.batch_with_lengths(lens, 40, cfg, seed=9)
    b64 = R.batch_with_lengths(lens, 64, cfg, seed=9)
    for k in b:
        b64[k][:, :40] = b[k]
    b64["input_ids"][:, 40:] = cfg.pad_id
    b64["token_type_ids"][:, 40:] = 0
    assert int(b64["attention_masks"][:, 40:].sum()) == 0
    f = lambda d: tuple(d[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))      # noqa: E731
    for varlen in (True, False):
        m.varlen = varlen
        try:
            assert same_bits(m.pair_latents(*f(b)), m.pair_latents(*f(b64))), (name, varlen)
        finally:
            m.varlen = True


# ------------------------------------------------------------------------------------------------ A.4 dispatch in eval mode
@pytest.mark.parametrize("case", ["zh24_B_129", "zh24_mix", "zh24_s64_mix", "en24_B_129"])
def test_dispatch_variants_against_the_oracle_and_each_other(case):
    name, N = R.EVAL_CASES[case][:2]
    m, b = model_of(name), gpu_batch(case)
    res = {}
    try:
        for varlen in (True, False):
            for cls_only in (True, False):
                m.varlen, m.cls_only_last = varlen, cls_only
                res[varlen, cls_only] = lat = m.pair_latents(*b, chunk=N).clone()
                assert (m._prepare_inputs(*b).pack is not None) == varlen
                check_rows(lat, case, (varlen, cls_only))
    finally:
        m.varlen, m.cls_only_last = True, True
    for k, v in res.items():                # to each other: the bound of test_token_packing_equals_padded_computation
        assert rel_err(v, res[True, True]) < 2e-3, (case, k)


# ------------------------------------------------------------------------------------------------ A.5 forward_terms against pair_latents
@pytest.mark.parametrize("case", ["zh24_B_129", "zh24_B_5", "en24_B_129", "zh32_B_129"])
def test_forward_terms_and_pair_latents_agree_bitwise(case):
    """In eval() both run the same encoder pass (inference workspace, no dropout) and the same latent kernel, carel_tail_latents."""
    name, N = R.EVAL_CASES[case][:2]
    m = model_of(name)
    bt = {k: v.cuda() for k, v in R.case_batch(case).items()}
    m.set_noise(*R.noise(name))
    out = m.forward_terms(bt["input_ids"], bt["attention_masks"], bt["token_type_ids"], bt["emo_labels"], bt["cau_labels"], bt["labels"],
                          bt["bow_reps"], 3)
    lat = torch.cat((out["mu_e"], out["lv_e"], out["mu_c"], out["lv_c"]), dim=1)
    assert same_bits(lat, m.pair_latents(*gpu_batch(case), chunk=N))


def test_chunk_loop_sees_a_weight_change():
    """The chunk loops bring the bf16 shadow of the weights up to date once, before the first chunk: an in-place change of the encoder's
    weights between two calls must show in the second, row by row against the oracle run on the changed weights."""
    name, case = "zh24", "zh24_two"
    cfg, opt, seed = R.MODELS[name]
    mcfg = M.encoder_config("zh", vocab_size=cfg.vocab_size, layers=cfg.layers, hidden_dropout=0.0, attn_dropout=0.0)
    m = M.DrlClassifier(M.make_opt(**vars(opt)), mcfg)
    m.load_state_dict(R.params(name))
    m.to("cuda").eval()
    b = gpu_batch(case)
    check_rows(m.pair_latents(*b, chunk=8), case)
    P2 = O.init_params(cfg, opt, seed=seed + 100)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.startswith("encoder.encoder.layer."):
                p.copy_(P2[k])
    P2 = {k: (v if k.startswith("encoder.encoder.layer.") else R.params(name)[k]) for k, v in P2.items()}
    lat = m.pair_latents(*b, chunk=8)
    cb = R.case_batch(case)
    with torch.no_grad():
        for q in (None, O.bf16_round):
            want = O.pair_latents(P2, cb["input_ids"], cb["attention_masks"], cb["token_type_ids"], cfg, opt, quant=q)
            assert float(R.row_rel(lat, want).max()) <= R.TOL_ROW_LATENT
    assert float(R.row_rel(lat, R.oracle_latents(case, False)).min()) > 10 * R.TOL_ROW_LATENT       # (the change is far outside the tolerance)


# ------------------------------------------------------------------------------------------------ B the three-space model
EN_CFG = O.EncoderConfig(layers=2, vocab_size=R.VOCAB, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)
ZH_CFG = O.EncoderConfig(layers=2, vocab_size=R.VOCAB)
EN_NS = (1, 9, 129)
_en = {}


def en_model(language):
    """(model, P, batch of 129 on the CPU, eps_e, eps_c, oracle logits [129]) of the three-space model, built once per language"""
    if language not in _en:
        cfg = EN_CFG if language == "en" else ZH_CFG
        opt = OE.OptEn(pair_bow_dim=R.V, dropout=0.0, language=language)
        P = OE.init_params(cfg, opt, seed=31)
        g = torch.Generator().manual_seed(32)
        eps_e, eps_c = torch.randn(opt.ec_dim, generator=g), torch.randn(opt.ec_dim, generator=g)
        lens = R._mix_lengths(max(EN_NS), 32)
        b = R.batch_with_lengths(lens, 32, cfg, seed=33)
        with torch.no_grad():
            raw = OE.pair_logits(dict(P, **{"pair_classifier.bias": torch.zeros_like(P["pair_classifier.bias"])}), b["input_ids"], b["attention_masks"],
                                 b["token_type_ids"], cfg, opt, eps_e, eps_c, quant=O.bf16_round).reshape(-1)
            # the oracle's logits on both sides of 0: bias = -median (the weight keeps its scale, and the logits the tolerances that
            # test_get_pair_preds_and_eval_forward holds them to)
            P = dict(P)
            P["pair_classifier.bias"] = torch.full_like(P["pair_classifier.bias"], -float(raw.median()))
            want = OE.pair_logits(P, b["input_ids"], b["attention_masks"], b["token_type_ids"], cfg, opt, eps_e, eps_c, quant=O.bf16_round).reshape(-1)
        mcfg = M.encoder_config(language, vocab_size=cfg.vocab_size, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps,
                                layers=cfg.layers, hidden_dropout=0.0, attn_dropout=0.0)
        kw = {k: v for k, v in vars(opt).items() if k in ME.DEFAULT_OPT}
        m = ME.DrlClassifier(ME.make_zh_opt(**kw) if language == "zh" else ME.make_opt(**kw), mcfg)
        m.load_state_dict(P)
        _en[language] = (m.to("cuda").eval(), P, b, eps_e, eps_c, want)
    return _en[language]


def en_logits(m, ids, att, tt, eps_e, eps_c, chunk):
    m.set_noise(torch.zeros(m.opt.con_dim), eps_e, eps_c)
    return m.pair_logits(ids, att, tt, chunk=chunk)


@pytest.mark.parametrize("N", EN_NS)
@pytest.mark.parametrize("language", ["en", "zh"])
def test_three_space_pair_logits_rows_slices_and_neighbours(language, N):
    m, P, b, eps_e, eps_c, want = en_model(language)
    cfg = EN_CFG if language == "en" else ZH_CFG
    ids, att, tt = (b[k][:N].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
    other = ids.clone()
    rs = np.random.RandomState(6)
    lens = att.sum(1).tolist()
    for i in range(1, N, 2):
        other[i, :lens[i]] = torch.from_numpy(rs.randint(2, cfg.vocab_size, size=lens[i])).cuda()
    for chunk in sorted({N, 128, 8}):
        got = en_logits(m, ids, att, tt, eps_e, eps_c, chunk).clone()
        assert got.shape == (N,)
        np.testing.assert_allclose(got.cpu().numpy(), want[:N].numpy(), rtol=5e-3, atol=2e-3)        # test_get_pair_preds_and_eval_forward's
        for s in range(0, N, chunk):
            alone = en_logits(m, ids[s:s + chunk], att[s:s + chunk], tt[s:s + chunk], eps_e, eps_c, chunk)
            assert same_bits(got[s:s + chunk], alone), (language, N, chunk, s)
        moved = en_logits(m, other, att, tt, eps_e, eps_c, chunk)
        assert same_bits(moved[0::2], got[0::2]), (language, N, chunk)
        if N > 1:
            assert not torch.equal(moved[1::2], got[1::2])


def test_three_space_get_pair_preds_zh_branch():
    """opt.language "zh": the nested python list of drl_classifier.py, round=False the probabilities, the default their rounding"""
    m, P, b, eps_e, eps_c, want = en_model("zh")
    N = 129
    args = tuple(b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
    prob = torch.sigmoid(want.double())
    m.set_noise(torch.zeros(m.opt.con_dim), eps_e, eps_c)
    raw = m.get_pair_preds(*args, round=False)
    assert isinstance(raw, list) and len(raw) == N and all(isinstance(r, list) and len(r) == 1 and isinstance(r[0], float) for r in raw)
    got = torch.tensor(raw, dtype=torch.float64).reshape(-1)
    logit = torch.log(got / (1 - got))
    np.testing.assert_allclose(logit.numpy(), want.numpy(), rtol=5e-3, atol=2e-3)
    m.set_noise(torch.zeros(m.opt.con_dim), eps_e, eps_c)
    preds = m.get_pair_preds(*args)
    assert preds == np.array(raw, dtype=np.float32).round().tolist() and set(np.array(preds).reshape(-1).tolist()) == {0.0, 1.0}
    far = (prob - 0.5).abs() > R.FAR
    assert int(far.sum()) >= 16 and set(prob.round()[far].tolist()) == {0.0, 1.0} and torch.equal(torch.tensor(preds, dtype=torch.float64).reshape(-1)[far], prob.round()[far])
    m_en, _, b_en, e_en, c_en, want_en = en_model("en")         # "en": the raw logits, a [N, 1] tensor
    m_en.set_noise(torch.zeros(m_en.opt.con_dim), e_en, c_en)
    t = m_en.get_pair_preds(*(b_en[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids")))
    assert torch.is_tensor(t) and t.shape == (N, 1)
