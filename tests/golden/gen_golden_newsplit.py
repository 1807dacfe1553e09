#!/usr/bin/env python3
"""Golden vectors for the host half of the new-split driver: runs the reference's OWN `read_ECPE_data` and `generate_self_train_data`
(AST-extracted from drl_classifier_ec_mmd_final_mul_newsplit_emnlp.py :833-958 and :961-1064 at generation time; nothing of their text
is stored) on two small ECPE-format files that this script writes itself (zh and en, the same eight documents) and stores inputs and
outputs in tests/golden/newsplit_small.json.  The documents cover: a cause after its emotion, cause == emotion, two causes of one
emotion, an emotion that is predicted but not true, a true emotion that is not predicted, a one-pair and a zero-pair document.
A document WITHOUT an ordered pair cannot come out of the reader (every document that has an emotion e also has the pair (e, e) or a
pair (e', c) with c <= e'), so `generate_self_train_data` is also run on a hand-built frame that has one, plus a document whose only
ordered pair sorts last.  The model is a stand-in whose get_pair_preds returns recorded probabilities (rounded when asked to); every
call runs under random.seed(42) and the next random.random() after it is stored, which pins the RNG consumption.
Skips (exit 0) when the reference checkout is absent.   python tests/golden/gen_golden_newsplit.py"""
import ast, json, os, random, re, sys, tempfile, types
import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CAREL_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))
SCRIPT = os.path.join(REF, "drl_classifier_ec_mmd_final_mul_newsplit_emnlp.py")

# (doc id, [(emotion clause, cause clause)], [(predicted emotion or 6, zh text, en text)])
DOCS = [
    (31, [(2, 3)], [(6, "天 气 突 然 变 冷", "The weather turned cold"), (3, "他 感 到 很 难 过", "He felt very sad"),
                    (6, "因 为 朋 友 要 走 了", "Because his friend was leaving"), (6, "火 车 已 经 进 站", "The train had arrived")]),
    (32, [(2, 2)], [(6, "她 打 开 了 信", "She opened the letter"), (0, "读 到 好 消 息 她 很 高 兴", "Reading the good news made her happy"),
                    (6, "然 后 去 做 饭", "Then she went to cook")]),
    (33, [(4, 2), (4, 4)], [(6, "会 议 开 始 了", "The meeting began"), (6, "经 理 取 消 了 奖 金", "The manager cancelled the bonus"),
                            (6, "大 家 都 沉 默", "Everyone fell silent"), (2, "被 骗 的 员 工 十 分 愤 怒", "The cheated workers were furious"),
                            (6, "散 会 了", "The meeting ended")]),
    (34, [(1, 1)], [(4, "听 到 巨 响 他 很 害 怕", "The loud bang frightened him"), (6, "他 跑 出 房 间", "He ran out of the room"),
                    (1, "邻 居 却 在 大 笑", "The neighbour was laughing"), (6, "原 来 是 鞭 炮", "It was only a firecracker")]),
    (35, [(2, 1), (3, 3)], [(6, "比 赛 输 了", "The match was lost"), (6, "队 员 们 很 失 望", "The players were disappointed"),
                            (5, "教 练 的 话 让 人 惊 讶", "The coach said something surprising")]),
    (36, [(2, 1)], [(6, "下 雨 了", "It started to rain"), (6, "孩 子 很 伤 心", "The child was upset"), (6, "天 黑 了", "It got dark")]),
    (37, [(1, 1)], [(0, "中 奖 让 他 欣 喜", "Winning the prize delighted him")]),
    (38, [(3, 1)], [(6, "考 试 没 有 通 过", "The exam was failed"), (6, "他 走 回 家", "He walked home"), (3, "他 很 沮 丧", "He was dejected")]),
]


def ecpe_text(language, test):
    """test: the emotion column holds the PREDICTED emotions (6 = none).  Otherwise the true ones: every emotion clause of the pair line
    has one (the reader looks it up for each pair) and no other clause does."""
    out = []
    for doc_id, pairs, clauses in DOCS:
        if not test:
            true = {e for e, _ in pairs}
            clauses = [((emo if emo != 6 else 4) if i + 1 in true else 6, zh, en) for i, (emo, zh, en) in enumerate(clauses)]
        out.append("%d %d" % (doc_id, len(clauses)))
        if language == "zh":
            out.append(", ".join("(%d,%d)" % p for p in pairs))
        else:
            out.append(" " + " ".join("(%d, %d)," % p for p in pairs))
        for i, (emo, zh, en) in enumerate(clauses):
            out.append("%d,%d,%s,%s" % (i + 1, emo, "null", zh if language == "zh" else en))
    return "\n".join(out) + "\n"


def reference_functions(language, bow_optimize):
    tree = ast.parse(open(SCRIPT, encoding="utf8").read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("read_ECPE_data", "generate_self_train_data")]
    ns = dict(pd=pd, re=re, random=random, randint=random.randint, torch=torch, device="cpu", print=lambda *a, **k: None,
              opt=types.SimpleNamespace(language=language, bow_optimize=bow_optimize))
    exec(compile(ast.Module(body=fns, type_ignores=[]), "<reference:newsplit>", "exec"), ns)
    return ns["read_ECPE_data"], ns["generate_self_train_data"]


def frame_rows(df):
    rows = []
    for _, r in df.iterrows():
        row = [r["pair"], int(r["label"]), None if r["emotion"] is None or pd.isna(r["emotion"]) else int(r["emotion"])]
        if "temporal_order" in df.columns:
            row.append(bool(r["temporal_order"]))
        rows.append(row)
    return rows


class Model:
    def __init__(self, scores):
        self.scores, self.round_seen = scores, []

    def eval(self):
        pass

    def get_pair_preds(self, ids, att, tt, round=True):
        self.round_seen.append(bool(round))
        return [[float(np.float32(s).round()) if round else float(s)] for s in self.scores]


def self_train_cases(frame_name, df, sizes, scores, generate):
    z = torch.zeros((max(len(df), 1), 4), dtype=torch.long)
    loader = [{"input_ids": z, "attention_masks": z + 1, "token_type_ids": z}]
    cases = []
    for strategy in ("threshold", "random", "extreme", "temporal_order", "temporal_order_modification"):
        for it in (0, 1):
            for r_flag in ("true", "false"):
                model = Model(scores)
                random.seed(42)
                out = generate(list(sizes), df, loader, model, strategy, it, r_flag)
                cases.append(dict(frame=frame_name, strategy=strategy, iteration=it, r_flag=r_flag, round_seen=model.round_seen,
                                  columns=list(out.columns), rows=frame_rows(out), next_random=random.random()))
    return cases


if __name__ == "__main__":
    if not os.path.exists(SCRIPT):
        print("reference checkout not found (set CAREL_REFERENCE); nothing generated")
        sys.exit(0)
    out = dict(meta=dict(pandas=pd.__version__, source="drl_classifier_ec_mmd_final_mul_newsplit_emnlp.py:833-958, :961-1064"),
               files={lang + ("_test" if test else "_train"): ecpe_text(lang, test) for lang in ("zh", "en") for test in (False, True)},
               reader=[], self_train_frames={}, self_train=[])
    tmp = tempfile.mkdtemp()
    frames = {}
    for lang in ("zh", "en"):
        for name in (lang + "_train", lang + "_test"):
            open(os.path.join(tmp, name + ".txt"), "w", encoding="utf8").write(out["files"][name])
        for bow_optimize in ("true", "false"):
            read, generate = reference_functions(lang, bow_optimize)
            for test in (False, True):
                path = os.path.join(tmp, lang + ("_test" if test else "_train") + ".txt")
                random.seed(42)
                df, sizes, unpred = read(path, test=test)
                out["reader"].append(dict(language=lang, bow_optimize=bow_optimize, test=test, file=lang + ("_test" if test else "_train"), columns=list(df.columns), rows=frame_rows(df),
                                          temporal_order_dtype=str(df["temporal_order"].dtype), docs_pair_size=[int(s) for s in sizes],
                                          num_unpred_emotions=int(unpred), next_random=random.random()))
                if test:
                    frames[(lang, bow_optimize)] = (df, sizes)
    _, generate = reference_functions("zh", "true")
    rs = random.Random(11)
    # frame 1: the zh test frame of the reader, fractional scores (two of them tied, one exactly 0.5)
    df, sizes = frames[("zh", "true")]
    scores = [round(rs.random(), 3) for _ in range(len(df))]
    scores[1], scores[2], scores[5] = 0.5, 0.5, scores[4]
    out["self_train_frames"]["reader_zh"] = dict(rows=frame_rows(df), sizes=[int(s) for s in sizes], scores=scores)
    out["self_train"] += self_train_cases("reader_zh", df, sizes, scores, generate)
    # frame 2: the en bow_optimize test frame (pairs keep their spaces)
    df, sizes = frames[("en", "true")]
    scores = [round(rs.random(), 3) for _ in range(len(df))]
    out["self_train_frames"]["reader_en_bow"] = dict(rows=frame_rows(df), sizes=[int(s) for s in sizes], scores=scores)
    out["self_train"] += self_train_cases("reader_en_bow", df, sizes, scores, generate)
    # frame 3: hand-built -- no ordered pair (3 pairs), the only ordered pair sorts last (3), one pair, zero pairs, ordered pair first of 4
    sizes = [3, 3, 1, 0, 4]
    order = [False, False, False, False, True, False, True, True, False, True, False]
    scores = [0.9, 0.2, 0.6, 0.7, 0.1, 0.8, 0.95, 0.91, 0.3, 0.3, 0.6]
    n = sum(sizes)
    df = pd.DataFrame({"pair": ["hand-pair-%02d" % i for i in range(n)], "label": [0] * n, "emotion": [(5 * i + 1) % 6 for i in range(n)],
                       "temporal_order": order})
    out["self_train_frames"]["hand"] = dict(rows=frame_rows(df), sizes=sizes, scores=scores)
    out["self_train"] += self_train_cases("hand", df, sizes, scores, generate)
    json.dump(out, open(os.path.join(HERE, "newsplit_small.json"), "w", encoding="utf8"), ensure_ascii=False, indent=1)
    print(len(out["reader"]), "reader cases;", len(out["self_train"]), "self-training cases;",
          sum(1 for c in out["self_train"] if c["rows"]), "non-empty")
