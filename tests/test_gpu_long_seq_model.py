"""The models at sequence lengths above 128 (the long-sequence attention kernels, csrc/attention_long.hip) against the CPU oracle:
zh DrlClassifier at max_len 256 (loss terms, every parameter gradient, packing, bitwise-reproducible gradients), RoBERTa at 512 (the
position-table boundary), a dense batch of more than 8 192 rows (GEMM dispatch, LayerNorm backward, the atomic embedding-gradient
fallback), max_len 200 (padded up to 224: exact) and SentenceTransformer (MPNet at 384, BERT at 200)."""
import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import sentence_transformer as ST_M
from oracle import carel_oracle as O
from oracle import carel_oracle_st as ST
from tests.test_gpu_model import TOL_TERM_BF16, TOL_KL_BF16, build, call, relnorm
from tests.test_gpu_triplet import CharTokenizer, MpnetCharTokenizer, _public

pytestmark = pytest.mark.gpu


def ragged_batch(B, S, cfg, opt, seed, lens):
    b = O.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=seed)
    att = torch.zeros((B, S), dtype=torch.long)
    for i, n in enumerate(lens):
        att[i, :n] = 1
    b["attention_masks"] = att
    b["input_ids"] = b["input_ids"] * att + cfg.pad_id * (1 - att)
    return b


def run_model(model, batch, it, eps):
    model.train()
    model.set_noise(*eps)
    loss = model(*call(model, batch, it))
    loss.backward()
    torch.cuda.synchronize()
    terms = {k: float(v) for k, v in model.last_terms().items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    return float(loss), terms, grads


def check_terms(terms, ref):
    for k in ("mmd", "emo", "cau", "pair", "kl_e", "kl_c", "rec"):
        r = float(ref[k])
        tol = TOL_KL_BF16 if k.startswith("kl") else TOL_TERM_BF16
        assert abs(terms[k] - r) <= tol * max(abs(r), 1e-3), (k, terms[k], r)


def check_grads(got, ref, worst_tol=4e-2, med_tol=1.5e-2):
    worst = {k: relnorm(got[k], g) for k, g in ref.items() if g is not None and float(g.norm()) > 1e-7 and not k.endswith("key.bias")}
    bad = {k: v for k, v in worst.items() if v > worst_tol}
    assert not bad, bad
    assert float(np.median(list(worst.values()))) < med_tol, sorted(worst.items(), key=lambda kv: -kv[1])[:4]


def eps_pair(opt, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(opt.ec_dim, generator=g), torch.randn(opt.ec_dim, generator=g)


def test_zh_max_len_256_terms_gradients_packing_and_reproducibility():
    cfg, opt = O.EncoderConfig(layers=2, vocab_size=1000), O.Opt(pair_bow_dim=257, dropout=0.0)
    lens = [256, 17, 140, 129, 200, 64, 255, 3]
    B, S = len(lens), 256
    batch = ragged_batch(B, S, cfg, opt, 7, lens)
    eps = eps_pair(opt)
    model, P = build(cfg, opt, 4)
    model.varlen = False
    _, terms, grads = run_model(model, batch, 3, eps)
    out, ref = O.loss_and_grads(P, batch, 3, cfg, opt, *eps)
    check_terms(terms, out)
    check_grads(grads, ref)
    # bitwise reproducible (B * S = 2 048 rows <= 8 192: the sorted embedding gradients too)
    model_b, _ = build(cfg, opt, 4)
    model_b.varlen = False
    _, terms2, grads2 = run_model(model_b, batch, 3, eps)
    assert terms2 == terms
    assert all(torch.equal(grads[k], grads2[k]) for k in grads), [k for k in grads if not torch.equal(grads[k], grads2[k])][:4]
    # token packing (padding skipped) equals the padded computation
    model2, _ = build(cfg, opt, 4)
    model2.varlen = True
    _, terms_p, grads_p = run_model(model2, batch, 3, eps)
    assert model2._last_call.pack is not None
    for k in terms:
        assert abs(terms[k] - terms_p[k]) <= 1e-3 * max(abs(terms[k]), 1e-3), (k, terms[k], terms_p[k])
    worst = max(relnorm(grads_p[k], grads[k]) for k in grads if float(grads[k].norm()) > 1e-6 and not k.endswith("key.bias"))
    assert worst < 2e-2, worst


def test_roberta_max_len_512_position_table_boundary():
    cfg = O.EncoderConfig(layers=2, vocab_size=1200, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)
    opt = O.Opt(language="en", pair_bow_dim=257, dropout=0.0)
    lens = [512, 300]                        # a full-length sample: position ids up to pad_id + 512 = 513, the last row of the table
    batch = ragged_batch(2, 512, cfg, opt, 9, lens)
    eps = eps_pair(opt)
    model, P = build(cfg, opt, 6)
    _, terms, grads = run_model(model, batch, 2, eps)
    out, ref = O.loss_and_grads(P, batch, 2, cfg, opt, *eps)
    check_terms(terms, out)
    check_grads(grads, ref)
    assert float(grads["encoder.embeddings.position_embeddings.weight"][513].norm()) > 0
    # one position more would run past the table
    with pytest.raises(L.CarelError, match="512"):
        model(*call(model, ragged_batch(2, 544, cfg, opt, 9, [544, 3]), 2))


def test_dense_batch_above_8192_rows():
    """B = 17, S = 512: 8 704 rows -- the GEMM plans and LayerNorm-backward layouts at that row count and the atomic embedding
    gradient (the sorted path stops at 8 192 rows)."""
    cfg, opt = O.EncoderConfig(layers=2, vocab_size=1000), O.Opt(pair_bow_dim=257, dropout=0.0)
    B, S = 17, 512
    batch = O.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=13)
    eps = eps_pair(opt)
    model, P = build(cfg, opt, 8)
    model.varlen = False
    _, terms, grads = run_model(model, batch, 1, eps)
    torch.set_num_threads(16)
    out, ref = O.loss_and_grads(P, batch, 1, cfg, opt, *eps)
    check_terms(terms, out)
    check_grads(grads, ref)


def test_max_len_200_runs_padded_to_224_with_identical_results():
    cfg, opt = O.EncoderConfig(layers=2, vocab_size=1000), O.Opt(pair_bow_dim=257, dropout=0.0)
    lens = [200, 5, 150, 99]
    b200 = ragged_batch(4, 200, cfg, opt, 17, lens)
    b224 = {k: v.clone() for k, v in b200.items()}
    for k, fill in (("input_ids", cfg.pad_id), ("attention_masks", 0), ("token_type_ids", 0)):
        b224[k] = torch.cat((b200[k], torch.full((4, 24), fill, dtype=b200[k].dtype)), 1)
    eps = eps_pair(opt)
    res = []
    for b in (b200, b224):
        model, P = build(cfg, opt, 2)
        model.varlen = False
        res.append(run_model(model, b, 1, eps))
        assert model._last_call.S == 224
    (l0, t0, g0), (l1, t1, g1) = res
    assert l0 == l1 and t0 == t1
    assert all(torch.equal(g0[k], g1[k]) for k in g0)
    out, ref = O.loss_and_grads(P, b200, 1, cfg, opt, *eps)
    check_terms(t0, out)


def _st_setup(variant, max_len):
    opt = O.Opt(pair_bow_dim=8)
    if variant == "mpnet":
        cfg = O.EncoderConfig(layers=2, vocab_size=300, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="mpnet", pad_id=1, rel_pos=True)
        mcfg, tok = M.encoder_config("mpnet", vocab_size=300, layers=2, hidden_dropout=0.0, attn_dropout=0.0), MpnetCharTokenizer()
    else:
        cfg = O.EncoderConfig(layers=2, vocab_size=300)
        mcfg, tok = M.encoder_config("zh", vocab_size=300, layers=2, hidden_dropout=0.0, attn_dropout=0.0), CharTokenizer()
    P = O.init_params(cfg, opt, seed=5)
    model = ST_M.SentenceTransformer(mcfg, tokenizer=tok, max_seq_length=max_len)
    model.load_state_dict({_public(model, k): v for k, v in P.items() if k.startswith("encoder.") and not (variant == "mpnet" and "token_type" in k)})
    model.to("cuda")
    rs = np.random.RandomState(3)
    sents = ["".join(chr(0x4E00 + int(c)) for c in rs.randint(0, 200, size=rs.randint(2, max_len + 20))) for _ in range(16)]
    sents[3] = "".join(chr(0x4E00 + int(c)) for c in rs.randint(0, 200, size=max_len + 5))     # truncated at max_len
    labels = rs.randint(0, 4, size=16).tolist()
    return cfg, P, model, sents, labels


@pytest.mark.parametrize("variant,max_len", [("mpnet", 384), ("bert", 200)])
def test_sentence_transformer_long_sequences(variant, max_len):
    cfg, P, model, sents, labels = _st_setup(variant, max_len)
    margin = 4.45 if variant == "bert" else 0.6
    with pytest.warns(UserWarning):
        feats = model.tokenize(sents)
    assert int(feats["attention_mask"].sum(1).max()) == max_len
    want = ST.encode(P, feats["input_ids"], feats["attention_mask"], feats["token_type_ids"], cfg)
    got = torch.from_numpy(model.encode(sents, batch_size=16))
    assert relnorm(got, want) < 1e-2
    # one step of fit() against the restatement's loop
    examples = [ST_M.InputExample(texts=[s], label=l) for s, l in zip(sents, labels)]
    loader = torch.utils.data.DataLoader(examples, shuffle=False, batch_size=16)
    loss = ST_M.losses.BatchSemiHardTripletLoss(model=model, margin=margin)
    model.fit(train_objectives=[(loader, loss)], epochs=1, warmup_steps=0, optimizer_params={"lr": 1e-3}, output_path=None)
    batches = [dict(input_ids=feats["input_ids"], attention_masks=feats["attention_mask"], token_type_ids=feats["token_type_ids"],
                    labels=torch.tensor(labels))]
    ref_losses, _, W = ST.fit_steps(P, batches, cfg, margin=margin, lr=1e-3, warmup_steps=0, total_steps=1)
    assert abs(model.last_fit.losses[0] - ref_losses[0]) <= 2e-3 * abs(ref_losses[0]), (model.last_fit.losses, ref_losses)
    sd = model.state_dict()
    probe = ["encoder.layer.0.attention.self.query.weight", "encoder.layer.1.output.dense.weight", "embeddings.position_embeddings.weight"]
    if variant == "mpnet":
        probe.append("encoder.relative_attention_bias.weight")
    for k in probe:
        d_ref = W["encoder." + k] - P["encoder." + k]
        d_got = sd[_public(model, "encoder." + k)].cpu() - P["encoder." + k]
        cos = float((d_ref.flatten() @ d_got.flatten()) / (d_ref.norm() * d_got.norm()))
        assert cos > 0.9 and 0.8 < float(d_got.norm() / d_ref.norm()) < 1.25, (k, cos, float(d_got.norm() / d_ref.norm()))
