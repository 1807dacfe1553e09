"""tests/ecpe_batches.py builds the run lengths that the embedding-gradient tests rely on (no GPU needed)."""
import numpy as np

from oracle import carel_oracle as O
from tests.ecpe_batches import BERT_SPECIAL, FIRST_CHAR_ID, ROBERTA_SPECIAL, char_ids, corpus_batch, run_lengths


def test_corpus_batches_hold_the_runs_of_real_data():
    cfg, opt = O.EncoderConfig(layers=1), O.Opt()
    batch, lens = corpus_batch(64, 128, cfg, opt, seed=1)
    ids, att = batch["input_ids"].numpy(), batch["attention_masks"].numpy()
    assert (att.sum(1) == lens).all() and (att[:, 0] == 1).all()
    assert ((np.arange(128)[None, :] < lens[:, None]) == (att == 1)).all()          # prefix masks
    assert (ids[att == 0] == BERT_SPECIAL["pad"]).all()
    runs = run_lengths(ids, att)
    assert runs[BERT_SPECIAL["cls"]] == 64 and runs[BERT_SPECIAL["sep"]] == 128
    assert 1000 < int(lens.sum()) <= 64 * 128 - 1000                                # the packed regime, thousands of padding rows
    assert max(n for i, n in runs.items() if i >= FIRST_CHAR_ID) >= 30               # the most frequent character
    assert (ids[att == 1][ids[att == 1] >= FIRST_CHAR_ID] < FIRST_CHAR_ID + len(char_ids())).all()
    again, _ = corpus_batch(64, 128, cfg, opt, seed=1)
    assert (again["input_ids"].numpy() == ids).all()                                # deterministic


def test_roberta_corpus_batches_use_roberta_special_ids():
    cfg = O.EncoderConfig(layers=1, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)
    batch, lens = corpus_batch(128, 64, cfg, O.Opt(language="en"), seed=2)
    ids, att = batch["input_ids"].numpy(), batch["attention_masks"].numpy()
    runs = run_lengths(ids, att)
    assert runs[ROBERTA_SPECIAL["cls"]] == 128 and runs[ROBERTA_SPECIAL["sep"]] == 256
    assert (ids[att == 0] == ROBERTA_SPECIAL["pad"]).all() and (lens <= 64).all()
