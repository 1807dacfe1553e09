"""Host side of the new-split driver (drl_classifier_ec_mmd_final_mul_newsplit_emnlp.py) against tests/golden/newsplit_small.json, which
holds what the reference's own read_ECPE_data (:833-958) and generate_self_train_data (:961-1064) return on small documents
(tests/golden/gen_golden_newsplit.py), plus prf_from_counts against sklearn.  No GPU."""
import json
import os
import random

import numpy as np
import pandas as pd
import pytest
import torch

from carel_vae_amd import data as D
from carel_vae_amd import training as T
from carel_vae_amd.drl_classifier import make_newsplit_opt

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newsplit_small.json"), encoding="utf8"))


def frame_rows(df):
    rows = []
    for _, r in df.iterrows():
        row = [r["pair"], int(r["label"]), None if r["emotion"] is None or pd.isna(r["emotion"]) else int(r["emotion"])]
        if "temporal_order" in df.columns:
            row.append(bool(r["temporal_order"]))
        rows.append(row)
    return rows


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("newsplit")
    out = {}
    for name, text in GOLD["files"].items():
        out[name] = str(root / (name + ".txt"))
        with open(out[name], "w", encoding="utf8") as f:
            f.write(text)
    return out


@pytest.mark.parametrize("case", GOLD["reader"], ids=lambda c: "%s-bow_%s-%s" % (c["language"], c["bow_optimize"], "test" if c["test"] else "train"))
def test_reader_matches_the_reference(case, files):
    random.seed(42)
    df, sizes, unpred = D.read_ECPE_data(files[case["file"]], test=case["test"], language=case["language"], newsplit=True,
                                         bow_optimize=case["bow_optimize"])
    assert list(df.columns) == case["columns"] == ["pair", "label", "emotion", "temporal_order"]
    assert frame_rows(df) == case["rows"]
    assert str(df["temporal_order"].dtype) == case["temporal_order_dtype"] == "bool"
    assert [int(s) for s in sizes] == case["docs_pair_size"] and unpred == case["num_unpred_emotions"]
    assert random.random() == case["next_random"]            # the training negatives consumed the same draws
    if case["language"] == "en" and case["bow_optimize"] == "true":
        assert all(" [SEP] " in p and " " in p.split(" [SEP] ")[0] for p in df["pair"])
    else:
        assert all(" " not in p for p in df["pair"])


def test_the_fixture_covers_the_cases_it_is_meant_to():
    t = next(c for c in GOLD["reader"] if c["language"] == "zh" and c["test"] and c["bow_optimize"] == "true")
    assert 0 in t["docs_pair_size"] and 1 in t["docs_pair_size"] and t["num_unpred_emotions"] == 2
    order = [r[3] for r in t["rows"] if r[1] == 1]
    assert True in order and False in order                   # a cause after its emotion, and one that is not
    hand = GOLD["self_train_frames"]["hand"]
    assert not any(r[3] for r in hand["rows"][:3])            # a document with no ordered pair
    got = {(c["strategy"], c["iteration"], c["r_flag"]) for c in GOLD["self_train"] if c["frame"] == "hand"}
    assert len(got) == 5 * 2 * 2


@pytest.mark.parametrize("language", ["zh", "en"])
def test_default_reader_output_is_unchanged(language, files):
    """Without the keyword: three columns, clauses glued, and the same rows as the opt-in form minus its fourth column."""
    for test in (False, True):
        path = files[language + ("_test" if test else "_train")]
        random.seed(42)
        df, sizes, unpred = D.read_ECPE_data(path, test=test, language=language)
        nxt = random.random()
        assert list(df.columns) == ["pair", "label", "emotion"]
        case = next(c for c in GOLD["reader"] if c["language"] == language and c["test"] == test and c["bow_optimize"] == "false")
        assert frame_rows(df) == [r[:3] for r in case["rows"]]
        assert sizes == case["docs_pair_size"] and unpred == case["num_unpred_emotions"] and nxt == case["next_random"]
        random.seed(42)
        df2, _, _ = D.read_ECPE_data(path, test=test, language=language, bow_optimize=True)      # bow_optimize alone changes nothing
        assert df2.equals(df)


class Recorded:
    """get_pair_preds returns recorded probabilities, rounded when asked to (what the fixture's stand-in did)."""

    def __init__(self, scores):
        self.scores, self.round_seen = scores, []

    def eval(self):
        pass

    def get_pair_preds(self, ids, att, tt, round=True):
        self.round_seen.append(bool(round))
        return [[float(np.float32(s).round()) if round else float(s)] for s in self.scores]


@pytest.mark.parametrize("case", GOLD["self_train"], ids=lambda c: "%s-%s-it%d-r_%s" % (c["frame"], c["strategy"], c["iteration"], c["r_flag"]))
def test_generate_self_train_data_matches_the_reference(case):
    fr = GOLD["self_train_frames"][case["frame"]]
    df = pd.DataFrame(fr["rows"], columns=["pair", "label", "emotion", "temporal_order"])
    z = torch.zeros((len(df), 4), dtype=torch.long)
    loader = [{"input_ids": z, "attention_masks": z + 1, "token_type_ids": z}]
    model = Recorded(fr["scores"])
    before = df.copy()
    random.seed(42)
    out = T.generate_self_train_data(list(fr["sizes"]), df, loader, model, case["strategy"], case["iteration"], case["r_flag"], device="cpu")
    nxt = random.random()
    assert list(out.columns) == case["columns"] == ["pair", "label", "emotion"]
    assert frame_rows(out) == case["rows"]
    assert model.round_seen == case["round_seen"]
    assert nxt == case["next_random"]                          # Python's RNG is left where the reference leaves it
    assert df.equals(before)


def test_older_call_form_and_refusals():
    fr = GOLD["self_train_frames"]["hand"]
    df = pd.DataFrame(fr["rows"], columns=["pair", "label", "emotion", "temporal_order"])
    z = torch.zeros((len(df), 4), dtype=torch.long)
    loader = [{"input_ids": z, "attention_masks": z + 1, "token_type_ids": z}]

    class ThreeArgs(Recorded):
        def get_pair_preds(self, ids, att, tt):               # the older models' signature: no round argument is passed without r_flag
            return [[float(s)] for s in self.scores]
    random.seed(42)
    out = T.generate_self_train_data(list(fr["sizes"]), df, loader, ThreeArgs(fr["scores"]), "random", device="cpu")
    want = next(c for c in GOLD["self_train"] if c["frame"] == "hand" and c["strategy"] == "random" and c["r_flag"] == "false" and c["iteration"] == 0)
    assert frame_rows(out) == want["rows"]
    with pytest.raises(ValueError):
        T.generate_self_train_data(list(fr["sizes"]), df.drop(columns=["temporal_order"]), loader, Recorded(fr["scores"]), "temporal_order", 0,
                                   "true", device="cpu")
    with pytest.raises(ValueError):
        T.generate_self_train_data(list(fr["sizes"]), df, loader, Recorded(fr["scores"]), "temporal_order_modification", device="cpu")


def test_newsplit_opt_and_paths():
    o = make_newsplit_opt()
    assert (o.source_domain, o.target_domain, o.self_strategy) == ("home", "education", "temporal_order_modification")
    assert (o.adapter, o.bow_optimize, o.predicted_emotion, o.round_up, o.confounding) == ("false", "true", "true", "true", "false")
    assert (o.language, o.ec_dim, o.epochs, o.batch_size, o.head_number, o.self_iteration, o.self_epochs) == ("zh", 24, 20, 64, 4, 50, 10)
    assert D.newsplit_paths(o) == ("data/ECPE_new_dataset/home.txt", "pair_data/predicted_emotion/source_home/education.txt")
    assert D.newsplit_paths(make_newsplit_opt(predicted_emotion="false"))[1] == "data/ECPE_new_dataset/education_test.txt"
    en = dict(language="en", source_domain="enecpe_num", target_domain="romance")
    assert D.newsplit_paths(make_newsplit_opt(**en)) == ("domains/Englishnovel_multiple/enecpe_num.txt",
                                                          "pair_data/predicted_emotion/source_enecpe_num/romance.txt")
    assert D.newsplit_paths(make_newsplit_opt(predicted_emotion="false", **en))[1] == "pair_data/emotion/romance_optimize.txt"
    assert D.newsplit_paths(make_newsplit_opt(predicted_emotion="false", bow_optimize="false", **en))[1] == "pair_data/emotion/romance.txt"


def test_dataset_counts_bow_tokens_for_english_with_the_optimised_vocabulary():
    df = pd.DataFrame({"pair": ["He felt very sad [SEP] Because his friend was leaving, sad!"], "label": [1], "emotion": [3]})
    bow = ["because", "felt", "sad", "sep", "zebra"]
    ds = D.ECPEDataset(df, tokenizer=None, bow=bow, language="en", bow_optimize="true")
    want = np.array([1, 1, 2, 1, 0], dtype=np.float32) / 5
    assert np.array_equal(ds.bow_representations[0], want)
    # everything else keeps the CJK filter + segmenter path: an English pair has no CJK character left, so no word is counted
    for kw in (dict(language="en", bow_optimize="false"), dict(language="zh", bow_optimize="true"), dict()):
        ds = D.ECPEDataset(df, tokenizer=None, bow=bow, segmenter=lambda t: t.split(), **kw)
        assert not ds.bow_representations[0].any()


def test_prf_from_counts_matches_sklearn():
    from sklearn.metrics import f1_score, precision_score, recall_score
    rs = np.random.RandomState(3)
    counts = rs.randint(0, 6, size=(40, 3, 3))
    counts[0] = 0                                              # every denominator zero
    counts[1, :, 0] = 0                                        # no true positive
    counts[2, :, 1:] = 0                                       # perfect
    counts[3, 0] = (0, 4, 0)                                   # predictions but no positive label
    counts[4, 0] = (0, 0, 4)                                   # positive labels but no prediction
    p, r, f = T.prf_from_counts(torch.from_numpy(counts))
    assert p.shape == r.shape == f.shape == (40, 3) and p.dtype == torch.float64
    for k in range(40):
        for g in range(3):
            tp, fp, fn = (int(v) for v in counts[k, g])
            y = [1] * tp + [0] * fp + [1] * fn + [0, 0]
            yhat = [1] * tp + [1] * fp + [0] * fn + [0, 0]
            kw = dict(average="binary", zero_division=0)
            want = (precision_score(y, yhat, **kw), recall_score(y, yhat, **kw), f1_score(y, yhat, **kw))
            got = (float(p[k, g]), float(r[k, g]), float(f[k, g]))
            assert got == pytest.approx(want, abs=1e-15, rel=1e-14), (k, g, got, want)
    tot = T.prf_from_counts(torch.from_numpy(counts).sum(1))    # overall figures: sum over the groups first
    assert tot[0].shape == (40,)
