"""Host-side checks of opt.train_adapter (the sentence adapters' weight gradients): the new symbols and struct against the header, the
option, the flat layout and get_params(), and the mathematics the kernels implement -- fp64 autograd of tests/adapter_restate.py against
central finite differences, and the exactly-zero key-bias gradient."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import drl_classifier_en as ME
from tests import adapter_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 768
MODES = ("entmax", "sparsemax", "raw")
LATENT = [n + t for n in ("emotion_mu", "emotion_log_var", "cause_mu", "cause_log_var") for t in (".weight", ".bias")]


def small_model(**kw):
    return M.DrlClassifier(M.make_opt(pair_bow_dim=211, **kw), M.encoder_config("zh", vocab_size=100, layers=1), seed=1)


def test_abi_stays_9_and_the_new_symbols_are_exported():
    lib = L.load()
    assert L.ABI_VERSION == 9 and lib.carel_abi_version() == 9
    for name in ("carel_adapter_wgrad_workspace_floats", "carel_adapter_backward_weights"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.carel_adapter_wgrad_workspace_floats(0, 1) == 0 and lib.carel_adapter_wgrad_workspace_floats(1, 0) == 0
    for B, G in ((1, 1), (7, 4), (64, 12)):         # dz [2G, B, 128], per-sample partials [2, B, G, 768], du [2, G, 768], dqv [2, 768]
        assert lib.carel_adapter_wgrad_workspace_floats(B, G) >= 2 * G * B * (128 + H) + 2 * G * H + 2 * H


def test_wgrad_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "carel_hip.h")).read()
    body = re.search(r"typedef struct carel_adapter_wgrad_args \{(.*?)\} carel_adapter_wgrad_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(void\*|int32_t)\s+(\w+)(?:\[(\d+)\])?", decl)
            assert m, decl
            fields.append((m.group(2), m.group(1), int(m.group(3) or 0)))
    assert [f[0] for f in fields] == [f[0] for f in L.AdapterWgradArgs._fields_]
    for (name, ctype, n), (_, ct) in zip(fields, L.AdapterWgradArgs._fields_):
        want = C.c_void_p if ctype == "void*" else C.c_int32
        assert ct is (want * n if n else want), name
    assert L.AdapterWgradArgs.work.offset == 16 * 8 and L.AdapterWgradArgs.accumulate.offset == 17 * 8
    assert C.sizeof(L.AdapterWgradArgs) == 18 * 8
    assert re.search(r"int64_t carel_adapter_wgrad_workspace_floats\(int32_t batch, int32_t heads\);", text)
    assert re.search(r"int carel_adapter_backward_weights\(const carel_adapter_args\* \w+, const carel_adapter_wgrad_args\* \w+, void\* stream\);", text)
    assert "#define CAREL_ABI_VERSION 9" in text


def test_option_validation():
    assert not hasattr(M.make_opt(), "train_adapter") and not hasattr(M.make_opt(adapter="entmax"), "train_adapter")
    assert small_model().train_adapter is False and small_model(adapter="entmax").train_adapter is False
    for v, want in ((True, True), (False, False), ("true", True), ("false", False)):
        assert small_model(adapter="entmax", train_adapter=v).train_adapter is want
    assert small_model(train_adapter=False).train_adapter is False and small_model(adapter="false", train_adapter="false").train_adapter is False
    for bad in ("yes", "True", 1, 0, None):
        with pytest.raises(L.CarelError, match="train_adapter"):
            small_model(adapter="entmax", train_adapter=bad)
    for kw in ({}, dict(adapter="false"), dict(adapter=False)):
        with pytest.raises(L.CarelError, match="train_adapter"):
            small_model(train_adapter=True, **kw)
    with pytest.raises(L.CarelError, match="MMD"):                   # other disentanglers: refused as before
        small_model(adapter="raw", train_adapter=True, disentangle="hsic")
    with pytest.raises(L.CarelError):                                # the three-space model has no adapters to train
        ME.DrlClassifier(ME.make_opt(pair_bow_dim=211, train_adapter=True), ME.encoder_config("en", vocab_size=100, layers=1))
    with pytest.raises(L.CarelError):
        ME.DrlClassifier(ME.make_opt(pair_bow_dim=211, adapter="entmax", train_adapter=True), ME.encoder_config("en", vocab_size=100, layers=1))


@pytest.mark.parametrize("mode", MODES)
def test_flat_layout_and_get_params(mode):
    frozen, trained = small_model(adapter=mode), small_model(adapter=mode, train_adapter="true")
    assert list(frozen.state_dict().keys()) == list(trained.state_dict().keys())
    for k, v in frozen.state_dict().items():
        assert torch.equal(v, trained.state_dict()[k]), k             # same initial draw
    want = ["%s_adapter.%s" % (s, n) for s in ("emotion", "cause") for n in M.ADAPTER_TRAINED[mode]]
    assert trained._adapter_train_names == want and frozen._adapter_train_names == []
    assert set(want) <= set(trained._adapter_names) and trained._adapter_names == frozen._adapter_names
    if mode == "raw":
        assert set(want) == set(trained._adapter_names)
    else:
        rest = {k.split(".", 1)[1] for k in set(trained._adapter_names) - set(want)}
        assert rest == {"in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "v_proj.weight", "v_proj.bias"}
    end = lambda m, k: m._offs[k] + m._named[k].numel()              # noqa: E731
    assert min(trained._offs[k] for k in want) >= trained._pair_hi              # after the pair range
    for k in want:
        assert end(trained, k) <= trained._n_opt, k
        assert frozen._offs[k] >= frozen._n_opt, k
    for k in [k for k in trained._adapter_names if k not in want] + LATENT:
        assert trained._offs[k] >= trained._n_opt, k
    grown = sum((trained._named[k].numel() + 63) & ~63 for k in want)
    assert trained._n_opt == frozen._n_opt + grown and trained._flat.numel() == frozen._flat.numel()
    for k in frozen._order:                                            # everything below the pair range keeps its place
        if frozen._offs[k] < frozen._pair_hi:
            assert trained._offs[k] == frozen._offs[k], k
    # get_params(): the reference's list, then the trained adapter tensors; one optimiser takes it
    name_of = lambda m: {id(p): k for k, p in m.named_parameters()}     # noqa: E731
    ref_names = [name_of(frozen)[id(p)] for p in frozen.get_params()]
    got_names = [name_of(trained)[id(p)] for p in trained.get_params()]
    assert got_names == ref_names + want
    assert not any("_adapter." in k or k in LATENT for k in ref_names)
    torch.optim.Adam(trained.get_params(), lr=1e-5)


def _case(mode, seed):
    g = torch.Generator().manual_seed(seed)
    B, S = 2, 32
    w = {}
    if mode == "raw":
        w["in_proj_weight"] = torch.randn(3 * H, H, generator=g, dtype=torch.float64) / math.sqrt(H)
        w["in_proj_bias"] = torch.randn(3 * H, generator=g, dtype=torch.float64) * 0.1
        w["out_proj.weight"] = torch.randn(H, H, generator=g, dtype=torch.float64) / math.sqrt(H)
        w["out_proj.bias"] = torch.randn(H, generator=g, dtype=torch.float64) * 0.1
    else:
        for n in ("q_proj", "k_proj"):
            w[n + ".weight"] = torch.randn(H, H, generator=g, dtype=torch.float64) / math.sqrt(H)
            w[n + ".bias"] = torch.randn(H, generator=g, dtype=torch.float64) * 0.1
        if mode == "entmax":
            w["k_proj.weight"] *= 4.0                # supports of a few tokens out of 32 (sparsemax has them at unit scale)
    q = torch.randn(H, generator=g, dtype=torch.float64)
    Hs = torch.randn(B, S, H, generator=g, dtype=torch.float64)
    d_out = torch.randn(B, H, generator=g, dtype=torch.float64)
    dirs = {k: [torch.randn(v.shape, generator=g, dtype=torch.float64) for _ in range(2)] for k, v in w.items()}
    return w, q, Hs, d_out, dirs


@pytest.mark.parametrize("mode", MODES)
def test_fp64_autograd_weight_gradients_match_central_differences(mode):
    """The loss sum(out * d_out) is piecewise smooth in the weights (C-infinity away from a change of support), so a central difference
    with step h along a unit direction errs by O(h^2 f''') plus the rounding of the two evaluations, at most eps * sum |out * d_out| / h
    (the loss is that sum of 2 x 768 terms).  Bound: 1e-6 of ||grad|| per unit direction plus that rounding floor (~2e-8 at h = 1e-5;
    it is what remains for the key bias, whose gradient is zero)."""
    w, q, Hs, d_out, dirs = _case(mode, seed=7)
    f = lambda ww: (R.adapter_out(Hs, q, ww, mode, 4)[0] * d_out).sum()      # noqa: E731
    leaves = {k: v.clone().requires_grad_() for k, v in w.items()}
    out, p = R.adapter_out(Hs, q, leaves, mode, 4)
    if mode != "raw":
        assert 1 < int((p > 0).sum(-1).min()) and int((p > 0).sum(-1).max()) < 32       # a real, partial support
    (out * d_out).sum().backward()
    h = 1e-5
    floor = torch.finfo(torch.float64).eps * float((out.detach() * d_out).abs().sum()) / h
    for k, ds in dirs.items():
        g = leaves[k].grad
        for d in ds:
            d = d / d.norm()
            plus, minus = dict(w), dict(w)
            plus[k], minus[k] = w[k] + h * d, w[k] - h * d
            with torch.no_grad():
                fd = float(f(plus) - f(minus)) / (2 * h)
            an = float((g * d).sum())
            assert abs(fd - an) <= 1e-6 * float(g.norm()) + floor, (k, fd, an, float(g.norm()))
    # the key bias: exactly zero mathematically (the normalisers are translation-invariant), rounding noise in fp64
    if mode == "raw":
        kb, kw = leaves["in_proj_bias"].grad[H:2 * H], leaves["in_proj_weight"].grad[H:2 * H]
    else:
        kb, kw = leaves["k_proj.bias"].grad, leaves["k_proj.weight"].grad
    assert float(kw.norm()) > 0
    assert float(kb.norm()) < 1e-12 * float(kw.norm()), (float(kb.norm()), float(kw.norm()))
