"""The embedding block's backward (carel_encoder_backward_embeddings) against float64, with a gradient of our own choosing.

The word / position table gradients of a training step come from fixed-order segment sums over keys `id << 13 | row` that the forward
pass sorted (csrc/ln.hip embed_sort_kernel, embed_segsum_kernel: one wave per run of equal ids, 64 keys per ballot), or from float atomics
where that path does not apply (more than 8192 rows, ids >= 2^19 - 1, no keys of this batch in the scratch).  Real batches
(tests/ecpe_batches.py) hold runs of 64 ([CLS]), 128 ([SEP]) and ~6 000 (padding) rows; here every row, padding and packed filler rows
included, gets an independent random gradient, so a dropped, doubled or misplaced row moves its table row by several percent.

Each case runs a 1-layer DrlClassifier forward (training mode), points the encoder arguments' dx at a random f32 [rows, 768] tensor and
calls carel_encoder_backward_embeddings exactly as a training step does.  The reference recomputes word[clamp(id)] + pos[pid] + type[tt]
-> LayerNorm -> embedding dropout in float64 from the same f32 tables, back-propagates dx through it and sums the table gradients with
index_add_.  Each touched table row is held to its own relative bound; untouched rows must be exactly zero; d type / d gamma / d beta are
compared as whole vectors.  Sorted-key cases also give bit-identical results over three calls and match the stand-alone atomic entry
point carel_embed_ln_bwd.  The last three tests break the pairing of forward and backward through the C ABI: the backward must then fall
back to the atomic path and still be right.

Bounds: a table row summed from up to 1 000 rows within 2e-6 of the float64 row, from more rows (the ~6 000-row padding run, the single
8192-row run) within 1e-5; whole vectors within 1e-6 -- about four times the worst values of one MI355X run (TOL_* below; `_report`
records them).  A dropped or doubled row in a 128-row run moves its table row by ~9 %."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from oracle import carel_oracle as O
from tests.ecpe_batches import corpus_batch
from tests.test_gpu_model import _report, call, relnorm

pytestmark = pytest.mark.gpu

H = 768
E = "encoder.embeddings."
WORD, POS, TYPE, LNG, LNB = (E + "word_embeddings.weight", E + "position_embeddings.weight", E + "token_type_embeddings.weight",
                             E + "LayerNorm.weight", E + "LayerNorm.bias")
KEYS = (WORD, POS, TYPE, LNG, LNB)
SORT_MAX = 8192
# measured worst on an MI355X (one run): 5.2e-7 (the 1 000-row run), 1.8e-6 (the 8192-row run), 1.5e-7 (the vectors)
TOL_ROW = 2e-6            # a table row summed from up to 1 000 rows, relative to the float64 row
TOL_ROW_LONG = 1e-5       # ... from more than 1 000 rows (the padding run, the single 8192-row run)
TOL_VEC = 1e-6            # d type_emb, d LayerNorm gamma / beta over the whole batch
BERT = O.EncoderConfig(layers=1)
ROBERTA = O.EncoderConfig(layers=1, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)


def _model(cfg, dropout, varlen, seed=3):
    """1-layer model; the word table is drawn with torch (init_params in numpy float64 would need ~7 GB of host memory at 2^19 rows)"""
    opt = O.Opt(language="en" if cfg.variant == "roberta" else "zh", pair_bow_dim=257, dropout=0.0)
    small = dataclasses.replace(cfg, vocab_size=min(cfg.vocab_size, 21128))
    P = O.init_params(small, opt, seed=seed)
    if small.vocab_size != cfg.vocab_size:
        P[WORD] = torch.randn(cfg.vocab_size, H, generator=torch.Generator().manual_seed(seed)) * 0.02
    mcfg = M.encoder_config("en" if cfg.variant == "roberta" else "zh", vocab_size=cfg.vocab_size, max_pos=cfg.max_pos,
                            type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps, layers=1, hidden_dropout=dropout, attn_dropout=dropout)
    model = M.DrlClassifier(M.make_opt(**vars(opt)), mcfg)
    model.load_state_dict(P)
    model.to("cuda")
    model.train()
    model.varlen = varlen
    return model, P, opt


def _forward(model, batch):
    """one training forward; -> the encoder arguments it ran with (the backward's own) and its call record"""
    loss = model(*call(model, batch, 3))
    del loss
    torch.cuda.synchronize()
    c = model._last_call
    return c.ea, c


def _forward_encoder(model, batch):
    """the encoder forward alone, through the model's own workspace and arguments (at B = 128 the classifier tail's decoder kernel has
    no room for the batch; the embedding block does not depend on it)"""
    b = {k: batch[k].cuda().contiguous() for k in ("input_ids", "attention_masks", "token_type_ids")}
    ids, att, tt = b["input_ids"], b["attention_masks"], b["token_type_ids"]
    B, S = ids.shape
    pack = model._pack_info(att, B, B, S)
    model._refresh_shadow()
    ea = model._encoder_args(ids, att, tt, model._workspace(B, S, False), B, S, False, True, 77, 0, pack)
    L.check(L.load().carel_encoder_forward(C.byref(ea), L.current_stream()), "carel_encoder_forward")
    torch.cuda.synchronize()
    return ea, types.SimpleNamespace(pack=pack, keep=b)


def _rows(ea):
    return int(ea.n_tokens) if ea.tok_row else int(ea.batch) * int(ea.seq_len)


def _tok_row(c):
    return None if c.pack is None else c.pack.tok_row.cpu().numpy().astype(np.int64)


def _dx(rows, seed):
    return torch.randn(rows, H, generator=torch.Generator().manual_seed(seed)).cuda()


def _backward(model, ea, dx):
    ea.dx = dx.data_ptr()
    L.check(L.load().carel_encoder_backward_embeddings(C.byref(ea), L.current_stream()), "carel_encoder_backward_embeddings")
    torch.cuda.synchronize()
    return {k: model._grad_view(k).detach().clone() for k in KEYS}


def _standalone(ea, dx):
    """the same gradients from carel_embed_ln_fwd / carel_embed_ln_bwd (float atomics) on the same arguments"""
    lib = L.load()
    rows, st = _rows(ea), L.current_stream()
    e = L.EmbedArgs()
    e.input_ids, e.token_type_ids, e.word_emb, e.pos_emb, e.type_emb = ea.input_ids, ea.token_type_ids, ea.word_emb, ea.pos_emb, ea.type_emb
    e.ln_gamma, e.ln_beta, e.ln_eps = ea.emb_ln_g, ea.emb_ln_b, ea.ln_eps
    e.batch, e.seq_len, e.hidden, e.vocab_size, e.max_pos, e.type_vocab = ea.batch, ea.seq_len, H, ea.vocab_size, ea.max_pos, ea.type_vocab
    e.roberta, e.pad_id = ea.roberta, ea.pad_id
    e.drop_seed, e.drop_idx_offset, e.drop_p = ea.drop_seed, ea.drop_row_offset * ea.seq_len * H, ea.hidden_dropout
    dev = dx.device
    x32, xb, stats = (torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev, dtype=torch.bfloat16),
                      torch.empty(rows, 2, device=dev))
    e.x_f32, e.x_bf16, e.stats = x32.data_ptr(), xb.data_ptr(), stats.data_ptr()
    e.tok_row, e.n_rows = ea.tok_row, (ea.n_tokens if ea.tok_row else 0)
    L.check(lib.carel_embed_ln_fwd(C.byref(e), st), "carel_embed_ln_fwd")
    out = {WORD: torch.zeros(ea.vocab_size, H, device=dev), POS: torch.zeros(ea.max_pos, H, device=dev),
           TYPE: torch.zeros(ea.type_vocab, H, device=dev), LNG: torch.zeros(H, device=dev), LNB: torch.zeros(H, device=dev)}
    part = torch.empty(lib.carel_embed_ln_bwd_blocks(rows) * (2 + ea.type_vocab) * H, device=dev)
    L.check(lib.carel_embed_ln_bwd(C.byref(e), dx.data_ptr(), *(out[k].data_ptr() for k in KEYS), part.data_ptr(), st), "carel_embed_ln_bwd")
    torch.cuda.synchronize()
    return out


def reference(P, cfg, ids, tt, tok_row, dx, seed, row_offset, p):
    """float64 gradients of the embedding block for output-row gradients dx [rows, 768]; the word table's as (touched ids, rows, counts)"""
    B, S = ids.shape
    orig = np.arange(B * S) if tok_row is None else tok_row
    t = np.nonzero(orig >= 0)[0]
    r = torch.from_numpy(orig[t])
    wid = ids.reshape(-1)[r].clamp(0, cfg.vocab_size - 1)
    pid = O.position_ids(ids, cfg).reshape(-1)[r].clamp(max=cfg.max_pos - 1)
    tid = tt.reshape(-1)[r].clamp(0, cfg.type_vocab - 1)
    x = P[WORD][wid].double() + P[POS][pid].double() + P[TYPE][tid].double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + cfg.ln_eps)
    xh = (x - mean) * rstd
    dy = dx.double().cpu()[torch.from_numpy(t)]
    if p > 0:
        idx = (np.uint64(row_offset * S * H) + r.numpy().astype(np.uint64)[:, None] * np.uint64(H)
               + np.arange(H, dtype=np.uint64)[None, :]).astype(np.uint32)
        dy = dy * torch.from_numpy(O.dropout_keep(seed, O.SITE_EMBED, idx, p).astype(np.float64) / (1.0 - p))
    dxh = dy * P[LNG].double()
    dh = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    uw, inv, cnt = torch.unique(wid, return_inverse=True, return_counts=True)
    return {WORD: (uw, torch.zeros(len(uw), H, dtype=torch.float64).index_add_(0, inv, dh), cnt),
            POS: torch.zeros(cfg.max_pos, H, dtype=torch.float64).index_add_(0, pid, dh),
            TYPE: torch.zeros(cfg.type_vocab, H, dtype=torch.float64).index_add_(0, tid, dh),
            LNG: (dy * xh).sum(0), LNB: dy.sum(0)}


def _row_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).numpy()


BUCKETS = ((1, 1), (2, 63), (64, 64), (65, 128), (129, 1000), (1001, SORT_MAX + 1024))


def check_tables(got, ref, name, tol=1.0):
    """every touched word / position row to its bound (scaled by tol), untouched rows exactly zero, the vectors as a whole;
    -> measured worst values"""
    uw, rw, cnt = ref[WORD]
    cnt = cnt.numpy()
    gw = got[WORD]
    err = _row_err(gw[uw.to(gw.device)], rw)
    bound = np.where(cnt > 1000, TOL_ROW_LONG, TOL_ROW) * tol
    worst = {"word_%d-%d" % (lo, hi): float(err[(cnt >= lo) & (cnt <= hi)].max()) for lo, hi in BUCKETS if ((cnt >= lo) & (cnt <= hi)).any()}
    bad = np.nonzero(err > bound)[0]
    assert len(bad) == 0, (name, "word rows", [(int(uw[i]), int(cnt[i]), float(err[i])) for i in bad[:8]])
    nz = (gw.abs().sum(1) > 0).cpu()
    touched = torch.zeros(gw.shape[0], dtype=torch.bool)
    touched[uw] = True
    assert torch.equal(nz, touched), (name, "word rows touched / nonzero", int(nz.sum()), int(touched.sum()))
    rp = ref[POS]
    tp = rp.abs().sum(1) > 0
    assert torch.equal((got[POS].abs().sum(1) > 0).cpu(), tp), (name, "position rows touched / nonzero")
    perr = _row_err(got[POS][tp.to(got[POS].device)], rp[tp])
    assert perr.max() <= TOL_ROW_LONG * tol, (name, "position row", int(np.argmax(perr)), float(perr.max()))
    worst["pos"] = float(perr.max())
    for k, short in ((TYPE, "type"), (LNG, "ln_gamma"), (LNB, "ln_beta")):
        worst[short] = e = relnorm(got[k], ref[k])
        assert e <= TOL_VEC * tol, (name, k, e)
    return worst


def _corpus_ids(cfg, B, S, seed):
    batch, _ = corpus_batch(B, S, cfg, O.Opt(pair_bow_dim=257), seed=seed)
    return batch


def _runs_batch(cfg):
    """all 8192 rows attended: 5 single ids below runs of 63, 64, 65, 127, 128, 129 and 1000 (sorted starts 5, 68, 132, 197, 324, 452,
    581: none a multiple of 64), every other row its own id; rows shuffled"""
    batch = O.synthetic_batch(64, 128, cfg, 257, seed=4, shape="A")
    runs = (63, 64, 65, 127, 128, 129, 1000)
    ids = list(range(700, 705))
    for i, n in enumerate(runs):
        ids += [710 + i] * n
    ids += list(range(3000, 3000 + SORT_MAX - len(ids)))
    ids = np.array(ids, dtype=np.int64)[np.random.RandomState(4).permutation(SORT_MAX)]
    batch["input_ids"] = torch.from_numpy(ids.reshape(64, 128))
    return batch


def _clamp_batch(cfg):
    """corpus ids with runs of -5 and 0 (both word row 0) and of vocab - 1 and vocab + 3 (both the last row), every row attended"""
    batch = _corpus_ids(cfg, 64, 128, 6)
    ids = batch["input_ids"].clone().reshape(-1)
    sel = np.random.RandomState(6).permutation(ids.numel())
    for i, v in enumerate((-5, 0, cfg.vocab_size - 1, cfg.vocab_size + 3)):
        ids[torch.from_numpy(sel[i * 50:(i + 1) * 50])] = v
    batch["input_ids"] = ids.reshape(64, 128)
    batch["attention_masks"] = torch.ones_like(batch["attention_masks"])
    return batch


def _one_id_batch(cfg):
    batch = O.synthetic_batch(64, 128, cfg, 257, seed=8, shape="A")
    batch["input_ids"] = torch.full((64, 128), 1234, dtype=torch.int64)
    return batch


def _sentinel_batch(cfg):
    batch = _corpus_ids(cfg, 64, 128, 9)
    batch["input_ids"][63, 127] = cfg.vocab_size - 1           # key (2^19 - 1) << 13 | 8191 = 0xFFFFFFFF, the filler sentinel
    batch["attention_masks"][63, 127] = 1
    return batch


# name: (config, dropout, varlen, batch builder, sorted keys expected)
CASES = {
    "bert_dense_corpus": (BERT, 0.0, False, lambda cfg: _corpus_ids(cfg, 64, 128, 1), True),
    "bert_dense_corpus_dropout": (BERT, 0.1, False, lambda cfg: _corpus_ids(cfg, 64, 128, 1), True),
    "bert_packed_corpus": (BERT, 0.0, True, lambda cfg: _corpus_ids(cfg, 64, 128, 1), True),
    "bert_packed_corpus_dropout": (BERT, 0.1, True, lambda cfg: _corpus_ids(cfg, 64, 128, 1), True),
    "bert_one_id_8192": (BERT, 0.0, False, _one_id_batch, True),
    "bert_runs_63_to_1000": (BERT, 0.0, False, _runs_batch, True),
    "bert_clamped_ids": (BERT, 0.0, False, _clamp_batch, True),
    "roberta_dense_corpus": (ROBERTA, 0.0, False, lambda cfg: _corpus_ids(cfg, 128, 64, 2), True),
    "roberta_packed_corpus": (ROBERTA, 0.0, True, lambda cfg: _corpus_ids(cfg, 128, 64, 2), True),
    "bert_dense_9216_rows_by_atomics": (BERT, 0.0, False, lambda cfg: _corpus_ids(cfg, 72, 128, 3), False),
    "bert_vocab_2e19_sentinel": (dataclasses.replace(BERT, vocab_size=1 << 19), 0.0, False, _sentinel_batch, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_embedding_backward_vs_float64(name):
    cfg, dropout, varlen, make, keyed = CASES[name]
    model, P, _ = _model(cfg, dropout, varlen)
    batch = make(cfg)
    ea, c = (_forward_encoder if batch["input_ids"].shape[0] > 64 else _forward)(model, batch)
    assert (c.pack is not None) == varlen, name
    rows = _rows(ea)
    dx = _dx(rows, 17)
    got = _backward(model, ea, dx)
    ref = reference(P, cfg, batch["input_ids"], batch["token_type_ids"], _tok_row(c), dx, int(ea.drop_seed), int(ea.drop_row_offset),
                    float(ea.hidden_dropout))
    worst = check_tables(got, ref, name)
    worst.update(rows=rows, longest_run=int(ref[WORD][2].max()))
    if keyed:
        for _ in range(2):                                  # fixed-order sums: bit-identical on every call
            again = _backward(model, ea, dx)
            for k in KEYS:
                assert torch.equal(again[k], got[k]), (name, k)
        atomic = _standalone(ea, dx)
        uw = ref[WORD][0]
        worst["vs_standalone_word"] = float(_row_err(got[WORD][uw.cuda()], atomic[WORD][uw.cuda()]).max())
        check_tables(atomic, ref, name + "_atomic")
    _report("embed_grad_" + name, worst)


# -- forward / backward pairing through the C ABI ------------------------------------------------------------------------------------


def _pairing_setup():
    model, P, _ = _model(BERT, 0.0, False)
    batch = _corpus_ids(BERT, 64, 128, 1)
    ea, c = _forward(model, batch)
    return model, P, batch, ea, c


def _ref_of(P, batch, dx):
    return reference(P, BERT, batch["input_ids"], batch["token_type_ids"], None, dx, 0, 0, 0.0)


def _copy(ea):
    return L.EncoderArgs.from_buffer_copy(ea)


def test_backward_after_forward_without_scratch_uses_no_stale_keys():
    """forward with scratch = NULL (no keys written), backward on a fresh zero-filled scratch: its all-zero 'keys' are no batch's"""
    model, P, batch, ea, _ = _pairing_setup()
    lib = L.load()
    e2 = _copy(ea)
    e2.scratch = None
    L.check(lib.carel_encoder_forward(C.byref(e2), L.current_stream()), "carel_encoder_forward")
    fresh = torch.zeros(lib.carel_encoder_scratch_bytes(int(ea.batch), int(ea.seq_len)), device="cuda", dtype=torch.uint8)
    e2.scratch = fresh.data_ptr()
    dx = _dx(_rows(ea), 21)
    check_tables(_backward(model, e2, dx), _ref_of(P, batch, dx), "fresh_scratch")


def test_backward_after_forward_of_another_batch_without_scratch():
    """forward + backward of batch X, then a forward of batch Y with scratch = NULL on the same act, then a backward with X's scratch:
    the gradients are Y's, not Y's rows summed by X's keys"""
    model, P, batch_x, ea, _ = _pairing_setup()
    lib = L.load()
    dx = _dx(_rows(ea), 22)
    check_tables(_backward(model, ea, dx), _ref_of(P, batch_x, dx), "batch_x")
    batch_y = _corpus_ids(BERT, 64, 128, 11)
    ids_y, att_y = batch_y["input_ids"].cuda().contiguous(), batch_y["attention_masks"].cuda().contiguous()
    e2 = _copy(ea)
    e2.input_ids, e2.attention_mask, e2.scratch = ids_y.data_ptr(), att_y.data_ptr(), None
    L.check(lib.carel_encoder_forward(C.byref(e2), L.current_stream()), "carel_encoder_forward")
    e2.scratch = ea.scratch
    check_tables(_backward(model, e2, dx), _ref_of(P, batch_y, dx), "batch_y")


def test_backward_without_side_stream_after_a_forward_that_sorted_on_it():
    """forward with overlap_wgrad = 1 (keys sorted on the side stream), backward with 0: ordered after the sort, and right"""
    model, P, batch, ea, _ = _pairing_setup()
    lib = L.load()
    e2 = _copy(ea)
    e2.overlap_wgrad = 1
    L.check(lib.carel_encoder_forward(C.byref(e2), L.current_stream()), "carel_encoder_forward")
    e2.overlap_wgrad = 0
    dx = _dx(_rows(ea), 23)
    e2.dx = dx.data_ptr()
    L.check(lib.carel_encoder_backward_embeddings(C.byref(e2), L.current_stream()), "carel_encoder_backward_embeddings")
    torch.cuda.synchronize()
    got = {k: model._grad_view(k).detach().clone() for k in KEYS}
    check_tables(got, _ref_of(P, batch, dx), "side_then_serial")
