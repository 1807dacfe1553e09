"""The padding / packing contract of DrlClassifier._prepare_inputs, the one way a batch gets to the encoder for every model path
(two-space and three-space training and inference, sentence fine-tune): CPU tensors, lengths given, nothing runs on a GPU."""
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import drl_classifier_en as E
from carel_vae_amd import sentence_transformer as ST


def _model(language="zh", **opt):
    return M.DrlClassifier(M.make_opt(pair_bow_dim=211, **opt), M.encoder_config(language, vocab_size=100, layers=1), seed=3)


def _batch(lens, S, pad_id=0):
    """ids in [2, 100) on the attended prefix of each row and pad_id behind it, the prefix mask, token types 1 on the second half."""
    g = torch.Generator().manual_seed(5)
    att = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(2, 100, (len(lens), S), generator=g) * att + pad_id * (1 - att)
    tt = (torch.arange(S)[None, :] >= S // 2).long() * att
    return ids, att, tt


LENS = [40, 7, 1, 33, 12]


def test_packed_batch_is_padded_to_the_tile_and_packed():
    m = _model()
    ids, att, tt = _batch(LENS, 40)
    c = m._prepare_inputs(ids, att, tt, LENS)
    assert (c.B, c.S, c.Bp) == (5, 64, 6)
    for t in (c.ids, c.att, c.tt):
        assert t.shape == (6, 64) and t.dtype == torch.long
    assert torch.equal(c.ids[:5, :40], ids) and torch.equal(c.att[:5, :40], att) and torch.equal(c.tt[:5, :40], tt)
    assert bool((c.ids[:5, 40:] == m.cfg.pad_id).all())                                  # the columns that round the length up
    assert int(c.att[:, 40:].abs().sum()) == 0 and int(c.tt[:, 40:].abs().sum()) == 0
    assert int(c.ids[5].abs().sum()) == 0 and int(c.att[5].abs().sum()) == 0 and int(c.tt[5].abs().sum()) == 0      # the filler row
    p = c.pack
    assert p.t_eff == 93 and p.n_tokens == 128
    assert p.cu.dtype == torch.int32 and p.cu.tolist() == [0, 40, 47, 48, 81, 93, 93]
    want = [b * 64 + pos for b, n in enumerate(LENS) for pos in range(n)]
    assert p.tok_row.dtype == torch.int32 and p.tok_row.shape == (128,)
    assert p.tok_row[:93].tolist() == want and bool((p.tok_row[93:] == -1).all())
    # without the lengths they are read from the mask: the same packing
    q = m._prepare_inputs(ids, att, tt).pack
    assert (q.t_eff, q.n_tokens) == (93, 128) and torch.equal(q.cu, p.cu) and torch.equal(q.tok_row, p.tok_row)
    # no token types: none are made up
    assert m._prepare_inputs(ids, att, None, LENS).tt is None


def test_full_batch_runs_dense():
    m = _model()
    ids, att, tt = _batch([32] * 4, 32)
    c = m._prepare_inputs(ids, att, tt, [32] * 4)
    assert c.pack is None and (c.B, c.S, c.Bp) == (4, 32, 4)
    assert torch.equal(c.ids, ids) and torch.equal(c.att, att) and torch.equal(c.tt, tt)


def test_roberta_pads_with_its_pad_id_and_keeps_its_length_limit():
    m = _model("en")
    assert m.cfg.pad_id == 1
    ids, att, _ = _batch(LENS, 40, pad_id=1)
    c = m._prepare_inputs(ids, att, None, LENS)
    assert (c.S, c.Bp) == (64, 6) and bool((c.ids[:5, 40:] == 1).all()) and int(c.att[:, 40:].abs().sum()) == 0
    assert int(c.ids[5].abs().sum()) == 0            # a filler row is zeros (masked out entirely), not pad_id
    # RoBERTa's position ids start at pad_id + 1: a table of 512 rows (BERT's) holds 510 positions, so 511 is refused; roberta-base's own
    # 514 rows hold 512, and 511 runs at 512
    short = M.DrlClassifier(M.make_opt(pair_bow_dim=211), M.encoder_config("en", vocab_size=100, layers=1, max_pos=512), seed=3)
    ids, att, _ = _batch([511], 511, pad_id=1)
    with pytest.raises(L.CarelError, match="sequence length must be at most 510"):
        short._prepare_inputs(ids, att, None, [511])
    assert m._prepare_inputs(ids, att, None, [511]).S == 512
    ids, att, _ = _batch([513], 513, pad_id=1)
    with pytest.raises(L.CarelError, match="sequence length must be at most 512"):
        m._prepare_inputs(ids, att, None, [513])


def test_sentence_adapter_keeps_its_lengths_and_runs_dense():
    m = _model(adapter="raw")
    ids, att, tt = _batch(LENS, 40)
    with pytest.raises(L.CarelError, match="with a sentence adapter the sequence length must be 32, 64, 96 or 128"):
        m._prepare_inputs(ids, att, tt, LENS)
    ids, att, tt = _batch(LENS, 64)
    c = m._prepare_inputs(ids, att, tt, LENS)
    assert c.pack is None and (c.B, c.S, c.Bp) == (5, 64, 6)          # an adapter attends to the padded positions too


def test_every_model_path_shares_the_one_front():
    base = M.DrlClassifier
    three = E.DrlClassifier(E.make_opt(pair_bow_dim=211), M.encoder_config("en", vocab_size=100, layers=1), seed=3)
    st = ST.SentenceTransformer(M.encoder_config("mpnet", vocab_size=100, layers=1), seed=3)
    for model in (three, st._m):
        for name in ("_prepare_inputs", "_run_encoder", "_overwriting_grads"):
            assert getattr(type(model), name) is getattr(base, name), (type(model).__name__, name)
            assert name not in vars(model)
