"""Host-side checks of the long-sequence support (ABI 9): new symbols, the attention struct against the header, the span-1024 MPNet
bucket map, the length rounding and limits of the models, and the embedding's position-table bound."""
import ctypes as C
import os
import re

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from oracle import carel_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi9_exports_the_long_sequence_entry_points():
    lib = L.load()
    assert L.ABI_VERSION == 9 and lib.carel_abi_version() == 9
    for name in ("carel_attention_bwd_workspace_bytes", "carel_relpos_expand_span", "carel_relpos_reduce_span"):
        assert hasattr(lib, name), name
    assert lib.carel_attention_bwd_workspace_bytes(64, 128, 1) == 0          # S <= 128: no workspace
    B, S = 16, 512
    delta = B * 12 * S * 4
    assert lib.carel_attention_bwd_workspace_bytes(B, S, 0) == delta
    assert lib.carel_attention_bwd_workspace_bytes(B, S, 1) == delta + B * 12 * 4 * 1024 * 4
    assert lib.carel_attention_bwd_workspace_bytes(3, 160, 1) >= 3 * 12 * 160 * 4 + 3 * 12 * 2 * 1024 * 4


def test_attention_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "carel_hip.h")).read()
    body = re.search(r"typedef struct carel_attn_args \{(.*?)\} carel_attn_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in decl.split(None, 1)[1].replace("*", " ").split(",")] if " " in decl else []
    names = [n.split()[-1] for n in names]
    assert names == [f[0] for f in L.AttnArgs._fields_]
    assert L.AttnArgs.workspace.offset % 8 == 0 and C.sizeof(L.AttnArgs) == L.AttnArgs.workspace_bytes.offset + 8


def test_span_1024_buckets_equal_transformers():
    got = M.mpnet_bucket_by_distance(1024)
    assert got.shape == (1024,) and got.dtype == torch.int32
    assert torch.equal(got.long(), O.mpnet_relative_position_bucket(torch.arange(-511, 513)))
    assert torch.equal(M.mpnet_bucket_by_distance(256).long(), O.mpnet_relative_position_bucket(torch.arange(-127, 129)))
    try:
        from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    except Exception:            # the oracle's restatement is pinned to transformers in tests/test_oracle_triplet.py
        return
    want = MPNetEncoder.relative_position_bucket(torch.arange(-511, 513), num_buckets=32, max_distance=128)
    assert torch.equal(got.long(), want)


def test_padded_length_rounding_and_limits():
    P = M.DrlClassifier._padded_len
    assert [P(s) for s in (32, 100, 128, 129, 160, 200, 384, 500, 512)] == [32, 128, 128, 160, 160, 224, 384, 512, 512]
    for bad in (0, 513, 544):
        with pytest.raises(L.CarelError, match="512"):
            P(bad)
    # RoBERTa / MPNet: ids from pad_id + 1, 514 rows -> 512 positions; a smaller table bounds the length
    assert P(512, max_pos=514, roberta=1, pad_id=1) == 512
    with pytest.raises(L.CarelError, match="at most 256"):
        P(300, max_pos=258, roberta=1, pad_id=1)
    with pytest.raises(L.CarelError, match="at most 256"):
        P(257, max_pos=256)
    # the batch pad keeps B * S a multiple of 128
    assert M.DrlClassifier._padded_batch(3, 160) == 4 and M.DrlClassifier._padded_batch(1, 384) == 1
    with pytest.raises(L.CarelError):
        M.DrlClassifier._padded_batch(2, 200)
    t = M.DrlClassifier._prep_ids(torch.ones((3, 200), dtype=torch.long), 4, 224, 7)
    assert t.shape == (4, 224) and int(t[0, 200:].unique()) == 7 and int(t[3].abs().sum()) == 0 and int(t[:3, :200].sum()) == 600


def test_sentence_adapters_keep_the_short_lengths():
    for mode in ("entmax15", "sparsemax", "raw"):
        with pytest.raises(L.CarelError, match="128"):
            M.DrlClassifier._padded_len(160, adapter=mode)
        with pytest.raises(L.CarelError, match="128"):
            M.DrlClassifier._padded_len(100, adapter=mode)
        assert M.DrlClassifier._padded_len(96, adapter=mode) == 96


def test_sentence_transformer_length_limit():
    from carel_vae_amd import sentence_transformer as S
    assert S.SentenceTransformer(M.encoder_config("zh", vocab_size=100, layers=1), max_seq_length=512).max_seq_length == 512
    with pytest.raises(L.CarelError, match="512"):
        S.SentenceTransformer(M.encoder_config("mpnet", vocab_size=100, layers=1), max_seq_length=513)


def test_embedding_rejects_positions_past_the_table():
    """carel_embed_ln_fwd: S <= max_pos (BERT), S <= max_pos - pad_id - 1 (RoBERTa / MPNet); checked before any launch."""
    lib = L.load()
    e = L.EmbedArgs()
    buf = torch.zeros(16, dtype=torch.float32)          # never read: the shape check comes first
    for f in ("input_ids", "word_emb", "pos_emb", "type_emb", "ln_gamma", "ln_beta"):
        setattr(e, f, buf.data_ptr())
    e.batch, e.hidden, e.vocab_size, e.type_vocab = 1, 768, 100, 1
    e.roberta, e.pad_id, e.max_pos, e.seq_len = 1, 1, 514, 513
    assert lib.carel_embed_ln_fwd(C.byref(e), None) == -2
    assert b"position table" in lib.carel_last_error()
    e.roberta, e.pad_id, e.max_pos, e.seq_len = 0, 0, 512, 513
    assert lib.carel_embed_ln_fwd(C.byref(e), None) == -2
