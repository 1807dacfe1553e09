"""The packed ECPE training step swept over its token-count dispatch regimes, against the bf16-emulating CPU oracle.

A packed batch reaches the encoder with its own token count T (the attended positions rounded up to a multiple of 128,
drl_classifier.py `_pack_info`), and the library picks kernels, K slices, slab-epilogue placement, weight-gradient splits and the
LayerNorm-backward layout as functions of T.  Each case below builds a B = 64, S = 128 batch whose per-sample lengths (2 .. 128) pack
to a chosen T and checks the whole training step (loss terms, every parameter gradient) against `oracle.carel_oracle` run with
`quant=O.bf16_hip`, at the bench-shape bounds of tests/test_gpu_model.py, plus checks that a norm over a whole tensor cannot dilute:

  * every real token has its own word id, so each touched row of the word-embedding gradient is ONE token's gradient: every row
    is held to a relative bound, and exactly the touched rows are nonzero (a dropped edge tile or a missing K slice at the end of T
    shows up as a handful of bad rows);
  * every sample's latent row (mu / log-var of both heads) and pooled row is held to a relative bound;
  * a second run of the same batch gives bit-identical gradients.

The model has three layers, not two: full layers 0 and 1 and the [CLS]-only layer 2.  With two layers the only full layer is layer 0,
which never defers its QKV data-gradient epilogue (it feeds the embedding backward), so the deferral into the next call's LayerNorm
backward (encoder.hip `defer_qkv` / `dx_in_slabs`) and the out-projection whose residual is recomputed from the LayerNorm below
(`plr1`) would go untested.  The model is shared by the cases, as in training: one batch after another with different T.

T values (tests/test_packed_dispatch.py derives the regimes from the library and fails if one has no T here):

    T     = 128 x   regime
    128     1       one row tile: out-proj / QKV / FFN1 on the 128x128 kernel; FFN2 forward and FFN1 data gradient 8 slabs, QKV data
                    gradient 4 slabs on the 128x128 kernel; weight gradients one per GEMM (the grouped launch needs T >= 256)
    256     2       split GEMMs move to the ping-pong kernel; grouped weight gradients without K-split tiles
    384     3       grouped launch still unsplit (odd multiple of 128)
    640     5       grouped launch: 2-way K split of its remainder tiles (odd multiple of 128; 512 is the other T of the regime)
    768     3 x 2   grouped launch 3-way split
    896     7       ... 3-way (odd)
    1024    8       ... 4-way (power of two)
    1152    9       ... 4-way (odd)
    1280    5 x 2   ... 5-way
    1408    11      ... 5-way (odd)
    1664    13      ... 6-way; odd multiple: weight-gradient K tiles do not halve evenly (1536 is the other T of the regime)
    1792    7 x 2   ... 7-way: the bench's packed shape (~1.8 k rows); FFN2 forward / FFN1 data gradient 4 slabs
    2048    16      ... 8-way; last T with one LayerNorm-backward row per wave
    2560    5 x 4   2 rows per wave (2176 .. 2560)
    2688    21      last T with 4 K slices on the K = 3072 / 2304 GEMMs; QKV / FFN1 forward on the 192-wide tile (odd)
    2816    11 x 2  2 K slices
    3072    3 x 8   single pass: the ping-pong kernel everywhere, no deferred epilogues (2944 .. 4096)
    4224    33      4 rows per wave in the LayerNorm backward (odd)
    5376    21 x 2  last T with the QKV forward on the 192-wide tile
    8192    64      QKV forward on the 288-wide tile (5504 .. 8192); 8128 attended tokens
    1792 with dropout 0.1 (hidden, attention and tail dropout: the oracle reproduces the counter-based masks)

The per-row and per-sample bounds are about twice the worst values measured over the sweep on an MI355X (recorded by `_report`)."""
import os

import numpy as np
import pytest
import torch

from oracle import carel_oracle as O
from tests.test_gpu_model import (TERMS, TOL_GRAD_BF16_EMU, TOL_GRAD_BF16_EMU_QK, TOL_KL_BF16, TOL_LOSS_OVER_SCALE, TOL_TERM_BF16, WEIGHTS,
                                  _report, build, call, relnorm)

pytestmark = pytest.mark.gpu

B, S = 64, 128
SWEEP_T = (128, 256, 384, 640, 768, 896, 1024, 1152, 1280, 1408, 1664, 1792, 2048, 2560, 2688, 2816, 3072, 4224, 5376, 8192)
DROPOUT_T = 1792
CASES = [(T, False) for T in SWEEP_T] + [(DROPOUT_T, True)]

# measured worst over the sweep on an MI355X: word row 1.23e-2 (T = 256), latent row 3.0e-3, pooled row 2.9e-3 (T = 768)
TOL_WORD_ROW = 2.5e-2     # worst row of the word-embedding gradient, relative to the oracle's row (one token each)
TOL_LATENT_ROW = 6e-3     # worst sample's latent row (mu_e | lv_e | mu_c | lv_c)
TOL_POOLED_ROW = 6e-3     # worst sample's pooled row
# the classifier heads' biases: their gradient is a sum of one term per sample, which can nearly cancel (T = 1792 here: the cause head's
# bias at 1.4e-2 of its own norm, every other tensor <= 5e-3); held to the same bound relative to the larger of their norm and a tenth
# of the norm of the per-sample terms' magnitudes (as the total loss is held on the scale of its terms)
HEAD_BIASES = ("emotion_classifier.bias", "cause_classifier.bias", "pair_classifier.bias")
WORD = "encoder.embeddings.word_embeddings.weight"


def lengths_for(T, seed):
    """64 per-sample lengths in [2, 128] whose sum packs to T rows: the attended-token count t_eff lies in (T - 128, T] (filler rows
    behind the last sample vary with T; T = 8192 stays one token short of a dense batch, which would not be packed)."""
    rs = np.random.RandomState(seed)
    t_eff = T - (T // 128 * 37) % 128
    t_eff = min(max(t_eff, T - 127, 2 * B), B * S - 1)
    assert (t_eff + 127) // 128 * 128 == T
    lens = np.full(B, 2, dtype=np.int64)
    w = rs.gamma(1.5, size=B)
    extra = t_eff - int(lens.sum())
    while extra > 0:
        room = S - lens
        p = w * (room > 0)
        add = np.minimum(rs.multinomial(extra, p / p.sum()), room)
        lens += add
        extra -= int(add.sum())
    assert int(lens.sum()) == t_eff and lens.min() >= 2 and lens.max() <= S
    return lens


def packed_batch(T, cfg, opt, seed):
    """ECPE-shaped labels / bag of words, prefix masks of lengths_for(T), and a distinct word id for every attended token."""
    lens = lengths_for(T, seed)
    batch = O.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=seed, shape="A")
    att = (torch.arange(S)[None, :] < torch.from_numpy(lens)[:, None]).to(torch.int64)
    rs = np.random.RandomState(seed + 1)
    ids = np.full((B, S), cfg.pad_id, dtype=np.int64)
    ids[att.numpy() == 1] = rs.permutation(np.setdiff1d(np.arange(cfg.vocab_size), [cfg.pad_id]))[:int(lens.sum())]
    batch["input_ids"], batch["attention_masks"] = torch.from_numpy(ids), att
    return batch, lens


def head_bias_scales(P, batch, pooled, it, opt, eps_e, eps_c, **kw):
    """|| sum_b |d loss / d bias|_b || for HEAD_BIASES: the oracle's tail with the bias repeated per sample (same forward values)"""
    Pg = dict(P)
    for k in HEAD_BIASES:
        Pg[k] = P[k].expand(B, -1).clone().requires_grad_(True)
    out = O.tail_forward(Pg, pooled, batch["emo_labels"], batch["cau_labels"], batch["labels"], batch["bow_reps"], it, opt, eps_e, eps_c, **kw)
    out["loss"].backward()
    return {k: float(Pg[k].grad.double().abs().sum(0).norm()) for k in HEAD_BIASES}


def grad_errors(got, grads, P, batch, out, opt, eps_e, eps_c, **kw):
    """relative error of every parameter gradient, per tensor; the head biases on the scale of their per-sample terms.
    -> (query / key projections, the rest)"""
    worst = {k: relnorm(got[k], gr) for k, gr in grads.items() if gr is not None and float(gr.norm()) > 1e-7 and not k.endswith("key.bias")}
    for k, sc in head_bias_scales(P, batch, out["pooled"], 3, opt, eps_e, eps_c, **kw).items():
        worst[k] = float((got[k].double() - grads[k].double()).norm()) / max(float(grads[k].double().norm()), 0.1 * sc)
    assert set(worst) <= set(got)
    qk = {k: v for k, v in worst.items() if ".attention.self.query." in k or ".attention.self.key." in k}
    return qk, {k: v for k, v in worst.items() if k not in qk}


def assert_grads(qk, rest, tag):
    """the bench-shape bounds (test_bench_shape_gradients_vs_the_bf16_emulating_oracle)"""
    bad = {k: v for k, v in rest.items() if v > TOL_GRAD_BF16_EMU}
    bad.update({k: v for k, v in qk.items() if v > TOL_GRAD_BF16_EMU_QK})
    assert not bad, (tag, bad)


def rows_relerr(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).numpy()


@pytest.fixture(scope="module")
def shared_model():
    cfg, opt = O.EncoderConfig(layers=3), O.Opt(dropout=0.0)
    model, P = build(cfg, opt, 0)
    model.train()
    return cfg, opt, model, P


def _run(model, batch, eps_e, eps_c):
    model.set_noise(eps_e, eps_c)
    for p in model.parameters():
        p.grad = None
    loss = model(*call(model, batch, 3))
    c = model._last_call
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    terms = {k: float(v) for k, v in model.last_terms().items()}
    return float(loss), terms, grads, c.buf.lat[:B].detach().cpu().clone(), c.buf.pooled[:B].detach().cpu().clone(), c


@pytest.mark.parametrize("T,dropout", CASES, ids=["T%d%s" % (T, "-dropout" if d else "") for T, d in CASES])
def test_packed_step_vs_bf16_emulating_oracle(shared_model, T, dropout):
    cfg, opt, model, P = shared_model
    if dropout:
        opt = O.Opt(dropout=0.1)
        model, P = build(cfg, opt, 0, train_dropout=True)
        model.train()
    assert cfg.vocab_size - 1 > B * S and (cfg.vocab_size, opt.pair_bow_dim) == (21128, 23771)
    batch, lens = packed_batch(T, cfg, opt, seed=T + (1 if dropout else 0))
    g = torch.Generator().manual_seed(T)
    eps_e, eps_c = torch.randn(opt.ec_dim, generator=g), torch.randn(opt.ec_dim, generator=g)
    loss, terms, got, lat, pooled, c = _run(model, batch, eps_e, eps_c)
    assert c.pack is not None and c.pack.n_tokens == T and c.pack.t_eff == int(lens.sum()), (T, c.pack and c.pack.n_tokens)
    seed = c.seed
    # the same batch again, with the same forward count (dropout masks): bit-identical
    model._fwd_count -= 1
    loss2, _, got2, lat2, _, c2 = _run(model, batch, eps_e, eps_c)
    assert c2.seed == seed and loss2 == loss
    assert torch.equal(lat2, lat)
    for k, v in got.items():
        assert torch.equal(got2[k], v), (T, k)

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    kw = dict(train=True, seed=seed) if dropout else {}
    out, grads = O.loss_and_grads(P, batch, 3, cfg, opt, eps_e, eps_c, quant=O.bf16_hip, **kw)
    lat_ref = torch.cat((out["mu_e"], out["lv_e"], out["mu_c"], out["lv_c"]), 1)

    # loss terms (tests/test_gpu_model.py bounds)
    for k in TERMS:
        r = float(out[k])
        tol = TOL_KL_BF16 if k.startswith("kl") else TOL_TERM_BF16
        assert abs(terms[k] - r) <= tol * max(abs(r), 1e-3), (T, k, terms[k], r)
    scale = sum(abs(WEIGHTS[k] * float(out[k])) for k in TERMS)
    assert abs(loss - float(out["loss"])) <= TOL_LOSS_OVER_SCALE * scale, (T, loss, float(out["loss"]), scale)

    qk, rest = grad_errors(got, grads, P, batch, out, opt, eps_e, eps_c, **kw)

    # per token: one word id per attended token -> one row of the word-embedding gradient per token
    touched = torch.zeros(cfg.vocab_size, dtype=torch.bool)
    touched[batch["input_ids"][batch["attention_masks"] == 1]] = True
    assert int(touched.sum()) == int(lens.sum())
    word_rows = rows_relerr(got[WORD][touched], grads[WORD][touched])
    # per sample
    lat_rows = rows_relerr(lat, lat_ref)
    pooled_rows = rows_relerr(pooled, out["pooled"])
    _report("packed_sweep_T%d%s" % (T, "_dropout" if dropout else ""),
            dict(T=T, t_eff=int(lens.sum()), worst_word_row=float(word_rows.max()), worst_word_row_at=int(word_rows.argmax()),
                 worst_latent_row=float(lat_rows.max()), worst_pooled_row=float(pooled_rows.max()), worst_qk=max(qk.values()),
                 worst_rest=max(rest.values()), worst_rest_key=max(rest, key=rest.get), median=float(np.median(list(qk.values()) + list(rest.values())))))

    assert_grads(qk, rest, T)
    assert torch.equal(got[WORD].abs().sum(1) > 0, touched), T                # exactly the touched rows are nonzero
    assert torch.equal(grads[WORD].abs().sum(1) > 0, touched), T
    assert word_rows.max() <= TOL_WORD_ROW, (T, float(word_rows.max()), int(np.argmax(word_rows)))
    assert lat_rows.max() <= TOL_LATENT_ROW, (T, float(lat_rows.max()), int(np.argmax(lat_rows)))
    assert pooled_rows.max() <= TOL_POOLED_ROW, (T, float(pooled_rows.max()), int(np.argmax(pooled_rows)))


# the same three-layer model on batches of the committed ECPE corpus (tests/ecpe_batches.py), packed (the default) and dense: a [CLS] run of
# 64 rows, a [SEP] run of 128 and frequent characters 40 - 60 times, where the sweep above gives every token its own id.  A word row is then a
# sum of one term per token with that id, which can nearly cancel: it is held to TOL_WORD_ROW relative to the larger of its norm and a
# tenth of the norm of the sum of its terms' magnitudes (as the head biases are).  The oracle runs on a word table expanded to one row per
# token (the same forward values), so that its gradient rows ARE the per-token terms; their index_add by id is the reference row.
MULT_BUCKETS = ((1, 1), (2, 63), (64, 64), (65, 127), (128, 128))


@pytest.mark.parametrize("varlen", [True, False], ids=["packed", "dense"])
def test_corpus_step_vs_bf16_emulating_oracle(shared_model, varlen):
    from tests.ecpe_batches import corpus_batch, run_lengths
    cfg, opt, model, P = shared_model
    batch, lens = corpus_batch(B, S, cfg, opt, seed=5)
    runs = run_lengths(batch["input_ids"].numpy(), batch["attention_masks"].numpy())
    assert runs[101] == B and runs[102] == 2 * B, (runs[101], runs[102])
    g = torch.Generator().manual_seed(5)
    eps_e, eps_c = torch.randn(opt.ec_dim, generator=g), torch.randn(opt.ec_dim, generator=g)
    model.varlen = varlen
    try:
        loss, terms, got, lat, pooled, c = _run(model, batch, eps_e, eps_c)
    finally:
        model.varlen = True
    assert (c.pack is not None) == varlen

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    ids = batch["input_ids"].reshape(-1)
    Pt = dict(P)
    Pt[WORD] = P[WORD][ids]
    out, grads = O.loss_and_grads(Pt, dict(batch, input_ids=torch.arange(B * S).reshape(B, S)), 3, cfg, opt, eps_e, eps_c, quant=O.bf16_hip)
    per_token = grads[WORD]
    grads[WORD] = torch.zeros(cfg.vocab_size, per_token.shape[1]).index_add_(0, ids, per_token)

    for k in TERMS:
        r = float(out[k])
        tol = TOL_KL_BF16 if k.startswith("kl") else TOL_TERM_BF16
        assert abs(terms[k] - r) <= tol * max(abs(r), 1e-3), (varlen, k, terms[k], r)
    scale = sum(abs(WEIGHTS[k] * float(out[k])) for k in TERMS)
    assert abs(loss - float(out["loss"])) <= TOL_LOSS_OVER_SCALE * scale, (varlen, loss, float(out["loss"]), scale)
    qk, rest = grad_errors(got, grads, P, batch, out, opt, eps_e, eps_c)

    att = batch["attention_masks"].reshape(-1) == 1
    touched = torch.unique(ids[att])
    mult = torch.tensor([runs[int(i)] for i in touched])
    mag = torch.zeros(cfg.vocab_size, per_token.shape[1], dtype=torch.float64).index_add_(0, ids[att], per_token[att].double().abs())
    ref_rows = grads[WORD][touched].double()
    den = torch.maximum(ref_rows.norm(dim=1), 0.1 * mag[touched].norm(dim=1))
    word_rows = ((got[WORD][touched].double() - ref_rows).norm(dim=1) / den.clamp_min(1e-30)).numpy()
    worst = {"word_mult_%d-%d" % (lo, hi): float(word_rows[((mult >= lo) & (mult <= hi)).numpy()].max())
             for lo, hi in MULT_BUCKETS if bool(((mult >= lo) & (mult <= hi)).any())}
    worst.update(worst_qk=max(qk.values()), worst_rest=max(rest.values()), worst_rest_key=max(rest, key=rest.get),
                 cls_row=float(word_rows[int((touched == 101).nonzero())]), sep_row=float(word_rows[int((touched == 102).nonzero())]))
    _report("corpus_step_%s" % ("packed" if varlen else "dense"), worst)

    assert_grads(qk, rest, varlen)
    assert word_rows.max() <= TOL_WORD_ROW, (varlen, float(word_rows.max()), int(touched[int(np.argmax(word_rows))]))
    untouched = torch.ones(cfg.vocab_size, dtype=torch.bool)
    untouched[ids] = False                                    # (the padding id, present in dense rows, is left out)
    assert float(got[WORD][untouched].abs().max()) == 0.0, varlen
