"""Batches with the token statistics of real ECPE training data, built from the committed corpus tests/golden/ecpe/society_num.txt.gz.

Every sample is `[CLS] emotion-clause [SEP] cause-clause [SEP]` (RoBERTa: `<s> e </s> c </s>`), one id per character, with a prefix
attention mask of its real length.  Character ids are the corpus frequency ranks from 672 upward (the first Chinese character of the
bert-base-chinese vocabulary), so the most frequent characters get the lowest ids.  A B = 64 batch therefore has a [CLS] run of 64 rows,
a [SEP] run of 128 and characters such as `的` 40 - 60 times: the runs of equal ids that the embedding tables' segment sums
(csrc/ln.hip embed_segsum_kernel) meet on every training step, which uniformly drawn ids (`synthetic_batch`) never produce.  Labels and
bag-of-words come from `oracle.carel_oracle.synthetic_batch`."""
import collections
import gzip
import os
import random
import tempfile

import numpy as np
import torch

from carel_vae_amd.data import read_ECPE_data
from oracle import carel_oracle as O

CORPUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecpe", "society_num.txt.gz")
FIRST_CHAR_ID = 672
BERT_SPECIAL = dict(cls=101, sep=102, pad=0)
ROBERTA_SPECIAL = dict(cls=0, sep=2, pad=1)
_cache = {}


def corpus_pairs():
    """(emotion clause, cause clause) strings of every pair of the corpus, in read_ECPE_data's row order (negatives drawn with seed 0)"""
    if "pairs" not in _cache:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "society_num.txt")
            with gzip.open(CORPUS, "rb") as f, open(path, "wb") as o:
                o.write(f.read())
            df, _, _ = read_ECPE_data(path, rng=random.Random(0))
        _cache["pairs"] = [tuple(p.split("[SEP]", 1)) for p in df["pair"]]
    return _cache["pairs"]


def char_ids():
    """character -> id: frequency rank over the corpus pairs (ties by code point) from FIRST_CHAR_ID upward"""
    if "ids" not in _cache:
        cnt = collections.Counter(ch for e, c in corpus_pairs() for ch in e + c)
        order = sorted(cnt, key=lambda ch: (-cnt[ch], ch))
        _cache["ids"] = {ch: FIRST_CHAR_ID + i for i, ch in enumerate(order)}
    return _cache["ids"]


def encode(e, c, S, special):
    """[CLS] e [SEP] c [SEP], the longer clause cut first until it fits in S"""
    cmap = char_ids()
    e, c = list(e), list(c)
    while len(e) + len(c) + 3 > S:
        if len(e) >= len(c):
            e.pop()
        else:
            c.pop()
    return [special["cls"]] + [cmap[ch] for ch in e] + [special["sep"]] + [cmap[ch] for ch in c] + [special["sep"]]


def corpus_batch(B, S, cfg, opt, seed=0):
    """B corpus pairs drawn with `seed`: input ids, prefix attention masks and their lengths; the rest of `synthetic_batch(..., seed)`"""
    roberta = cfg.variant == "roberta"
    special = ROBERTA_SPECIAL if roberta else BERT_SPECIAL
    assert special["pad"] == cfg.pad_id, (special, cfg.pad_id)
    pairs = corpus_pairs()
    assert FIRST_CHAR_ID + len(char_ids()) <= cfg.vocab_size, (len(char_ids()), cfg.vocab_size)
    rs = np.random.RandomState(seed)
    pick = rs.choice(len(pairs), size=B, replace=False)
    ids = np.full((B, S), special["pad"], dtype=np.int64)
    lens = np.zeros(B, dtype=np.int64)
    for b, i in enumerate(pick):
        seq = encode(pairs[i][0], pairs[i][1], S, special)
        ids[b, :len(seq)] = seq
        lens[b] = len(seq)
    batch = O.synthetic_batch(B, S, cfg, opt.pair_bow_dim, seed=seed, shape="A")
    batch["input_ids"] = torch.from_numpy(ids)
    batch["attention_masks"] = (torch.arange(S)[None, :] < torch.from_numpy(lens)[:, None]).to(torch.int64)
    return batch, lens


def run_lengths(ids, att=None):
    """id -> number of attended rows carrying it"""
    ids = ids if att is None else ids[att == 1]
    u, n = np.unique(np.asarray(ids).reshape(-1), return_counts=True)
    return dict(zip(u.tolist(), n.tolist()))
