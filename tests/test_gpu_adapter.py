"""Sentence adapters of the EMNLP scripts (drl_classifier_ec_mmd_final_mul_emnlp.py): the HIP kernels (csrc/adapter.hip) against a
float64 restatement of the reference's own computation (tests/adapter_restate.py), and their wiring into DrlClassifier."""
import ctypes as C
import math

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import ops
from carel_vae_amd import training as T
from oracle import carel_oracle as O
from tests import adapter_restate as R

pytestmark = pytest.mark.gpu

H = 768
MODES = [("entmax", 1), ("sparsemax", 1), ("raw", 4), ("raw", 12)]


def relnorm(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _weights(mode, g, kscale):
    w = {}
    if mode == "raw":
        w["in_proj_weight"] = torch.randn(3 * H, H, generator=g, dtype=torch.float64) / math.sqrt(H)
        w["in_proj_weight"][H:2 * H] *= kscale
        w["in_proj_bias"] = torch.randn(3 * H, generator=g, dtype=torch.float64) * 0.1
        w["out_proj.weight"] = torch.randn(H, H, generator=g, dtype=torch.float64) / math.sqrt(H)
        w["out_proj.bias"] = torch.randn(H, generator=g, dtype=torch.float64) * 0.1
    else:
        for n in ("q_proj", "k_proj"):
            w[n + ".weight"] = torch.randn(H, H, generator=g, dtype=torch.float64) / math.sqrt(H)
            w[n + ".bias"] = torch.randn(H, generator=g, dtype=torch.float64) * 0.1
        w["k_proj.weight"] *= kscale
    return {k: v.float().double() for k, v in w.items()}         # exactly representable in f32


def _kernel_weights(w, mode):
    d = {k: v.float().cuda().contiguous() for k, v in w.items()}
    if mode == "raw":
        wi, bi = d["in_proj_weight"], d["in_proj_bias"]
        return dict(q_w=wi[:H], q_b=bi[:H], k_w=wi[H:2 * H], v_w=wi[2 * H:], v_b=bi[2 * H:], o_w=d["out_proj.weight"], o_b=d["out_proj.bias"])
    return dict(q_w=d["q_proj.weight"], q_b=d["q_proj.bias"], k_w=d["k_proj.weight"])


def _inputs(B, S, seed):
    """H [B, S, 768] (f32 values) with, when B allows: an exact tie at the top, a constant sample, a sample with a dominant row."""
    g = torch.Generator().manual_seed(seed)
    Hs = torch.randn(B, S, H, generator=g).double()
    if B >= 3:
        Hs[1, 3] = Hs[1, 0]                 # two identical rows: tied scores
        Hs[1, 9] = Hs[1, 0]
        Hs[2] = Hs[2, 0]                    # every row identical: a constant score row
    if B >= 4:
        Hs[3, 5] *= 8.0                     # one dominant row: a support of (nearly) one under the sparse modes
    return Hs


def _margin_ok(scores, mode):
    """Per sample: every score at least 1e-3 from the support threshold (the sparsemax backward is discontinuous there)."""
    x = scores
    p = R.sparsemax(x) if mode == "sparsemax" else R.entmax15(x)
    if mode == "entmax":
        x = (scores - scores.max(-1, keepdim=True).values) / 2
    tau = torch.where(p > 0, x - (p.sqrt() if mode == "entmax" else p), torch.full_like(x, float("nan"))).nanmean(-1, keepdim=True)
    d = (x - tau).abs()
    const = (scores == scores[..., :1]).all(-1, keepdim=True)
    return ((d > 1e-3) | (x == x.max(-1, keepdim=True).values) | const).all(-1)


def _run_kernels(mode, G, Hs, Bp, qs, ws, d_out):
    B, S, _ = Hs.shape
    x = torch.zeros((Bp * S, H), device="cuda", dtype=torch.float32)
    x[:B * S] = Hs.reshape(B * S, H).float().cuda()
    buf = ops.AdapterBuffers(B, S, G, x.device)
    u = torch.empty((2, G, H), device="cuda", dtype=torch.float32)
    dx = torch.full((Bp * S, H), float("nan"), device="cuda", dtype=torch.float32)
    qd = [q.float().cuda().contiguous() for q in qs]
    a = ops.adapter_args(mode, G, qd, [_kernel_weights(w, mode) for w in ws], u, buf, Bp, x=x, dx=dx)
    ops.adapter_build_u(a)
    ops.adapter_forward(a)
    buf.d_out.copy_(d_out.float())
    ops.adapter_backward(a)
    torch.cuda.synchronize()
    return buf.out.clone(), dx.clone()


@pytest.mark.parametrize("mode,G", MODES)
@pytest.mark.parametrize("S", [32, 96, 128])
@pytest.mark.parametrize("B", [1, 7, 64])
@pytest.mark.parametrize("kscale", [1.0, 40.0])
def test_kernels_vs_float64_restatement(mode, G, S, B, kscale):
    g = torch.Generator().manual_seed(100 * S + B)
    ws = [_weights(mode, g, kscale) for _ in range(2)]
    qs = [torch.randn(H, generator=g).double() for _ in range(2)]
    Hs = _inputs(B, S, seed=S + B)
    Bp = B + 1
    d_out = torch.randn(2, B, H, generator=g).double()
    out, dx = _run_kernels(mode, G, Hs, Bp, qs, ws, d_out)
    out2, dx2 = _run_kernels(mode, G, Hs, Bp, qs, ws, d_out)
    assert torch.equal(out, out2) and torch.equal(dx, dx2), "repeat launch not bitwise identical"
    assert bool((dx[B * S:] == 0).all()), "filler rows must be zero"
    Hr = Hs.clone().requires_grad_()
    keep = torch.ones(B, dtype=torch.bool)
    total = 0.0
    for side in range(2):
        ref, p = R.adapter_out(Hr, qs[side], ws[side], mode, G)
        assert relnorm(out[side], ref.detach()) <= 1e-5, (side, relnorm(out[side], ref.detach()))
        if mode == "sparsemax":
            with torch.no_grad():
                qp = qs[side] @ ws[side]["q_proj.weight"].T + ws[side]["q_proj.bias"]
                sc = (Hs @ ws[side]["k_proj.weight"].T + ws[side]["k_proj.bias"]) @ qp / math.sqrt(H)
            keep &= _margin_ok(sc, mode)
        total = total + (ref * d_out[side]).sum()
    total.backward()
    dref = Hr.grad.reshape(B, S, H)
    got = dx[:B * S].reshape(B, S, H).cpu()
    if B > 1:
        assert int(keep.sum()) >= B // 2
    if keep.any():
        assert relnorm(got[keep], dref[keep]) <= 1e-4, relnorm(got[keep], dref[keep])
    if kscale > 1 and mode != "raw":         # narrow supports: a few tokens
        with torch.no_grad():
            ref, p = R.adapter_out(Hs, qs[0], ws[0], mode, G)
        assert float((p > 0).sum(-1).double().median()) < S / 4


# ---------------------------------------------------------------------------------------------- the model
CFG = O.EncoderConfig(layers=2, vocab_size=1000)


def _model(mode, heads=4, seed=3, **kw):
    opt = M.make_opt(pair_bow_dim=257, dropout=0.0, adapter=mode, head_number=heads, **kw)
    m = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=1000, layers=2, hidden_dropout=0.0, attn_dropout=0.0), seed=seed)
    if mode == "entmax":                     # supports of a few tokens on some samples: scale the key projections
        with torch.no_grad():
            m.emotion_adapter.k_proj.weight.mul_(30.0)
    return m.to("cuda").train()


def _batch(B, S, seed=21):
    b = O.synthetic_batch(B, S, CFG, 257, seed=seed, shape="B")
    return {k: v.cuda() for k, v in b.items()}


def _call(b, it=3):
    return (b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], it)


def _noise(D=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(D, generator=g), torch.randn(D, generator=g)


def _copy_dev(ptr, n_floats):
    """A copy of n_floats f32 at a device pointer (a one-slab reduction is a plain copy)."""
    out = torch.empty(n_floats, device="cuda", dtype=torch.float32)
    L.check(L.load().carel_slab_reduce_f32(C.c_void_p(ptr), out.data_ptr(), n_floats, 1, 0, L.current_stream()), "copy")
    return out


def _heads_ref(model, a_e, a_c):
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    f = lambda n, x: x @ sd[n + ".weight"].T + sd[n + ".bias"]
    return dict(mu_e=f("emotion_mu", a_e), lv_e=f("emotion_log_var", a_e), mu_c=f("cause_mu", a_c), lv_c=f("cause_log_var", a_c))


def _adapter_ref(model, Hs):
    sd = model.state_dict()
    G = model.head_number
    e = R.adapter_out(Hs, model.emotion_q.double().cpu().reshape(-1), R.adapter_weights(sd, "emotion"), model.adapter, G)[0]
    c = R.adapter_out(Hs, model.cause_q.double().cpu().reshape(-1), R.adapter_weights(sd, "cause"), model.adapter, G)[0]
    return e, c


@pytest.mark.parametrize("mode,heads", [("entmax", 4), ("sparsemax", 4), ("raw", 4)])
@pytest.mark.parametrize("B,S", [(8, 128), (7, 96)])
def test_wiring_on_the_models_own_last_hidden_states(mode, heads, B, S, monkeypatch):
    _wiring(mode, heads, B, S, monkeypatch)


@pytest.mark.parametrize("mode,heads", [("sparsemax", 4), ("raw", 6)])
def test_wiring_at_length_64_and_a_head_count_of_six(mode, heads, monkeypatch):
    """The model itself across S = 64 (the length at which no lane of wave_normalise owns a second position) and the NV = 12
    instantiation of the raw kernels, which no other model-level test launches."""
    _wiring(mode, heads, 5, 64, monkeypatch)


def _wiring(mode, heads, B, S, monkeypatch):
    model = _model(mode, heads)
    b = _batch(B, S)
    Bp = model._padded_batch(B, S)
    # fp32 debug forward: the adapters + heads on its own x (dense [Bp*S, 768])
    model.debug_fp32 = True
    model.set_noise(*_noise())
    out = model.forward_terms(*_call(b))
    x = model._ws[("f32", Bp, S)].x[:B * S].double().cpu().reshape(B, S, H)
    a_e, a_c = _adapter_ref(model, x)
    assert relnorm(out["adapter_e"], a_e) <= 1e-5 and relnorm(out["adapter_c"], a_c) <= 1e-5
    for k, v in _heads_ref(model, a_e, a_c).items():
        assert relnorm(out[k], v) <= 1e-5, k
    # training step (bf16 encoder): dx_last against autograd of the restatement, given the tail's d head_in
    model.debug_fp32 = False
    model.set_noise(*_noise())
    loss = model(*_call(b))
    c = model._last_call
    x = _copy_dev(L.load().carel_encoder_x_last(C.byref(c.ea)), Bp * S * H).view(Bp, S, H)[:B].double().cpu().requires_grad_()
    seen = {}
    real = ops.adapter_backward

    def spy(a):              # dx_last as the encoder backward receives it (that backward then reuses the buffer)
        real(a)
        seen["dx"] = _copy_dev(a.dx_f32, Bp * S * H)
    monkeypatch.setattr(ops, "adapter_backward", spy)
    loss.backward()
    d_in = model._ws[("adapter", B, S)].d_out.double().cpu()
    a_e, a_c = _adapter_ref(model, x)
    ((a_e * d_in[0]).sum() + (a_c * d_in[1]).sum()).backward()
    dx = seen["dx"].view(Bp * S, H).double().cpu()
    assert relnorm(dx[:B * S].view(B, S, H), x.grad) <= 1e-4
    assert bool((dx[B * S:] == 0).all())
    # d head_in from the tail: the latent heads' data gradient of dlat (carel_tail_workspace layout: dz_core, dlat_direct, dlat)
    D = 24
    al = lambda n: (n + 63) // 64 * 64
    o = al(B * 2 * D) + al(B * 4 * D)
    dlat = c.buf.work[o:o + B * 4 * D].view(B, 4 * D).double().cpu()
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    want_e = dlat[:, :D] @ sd["emotion_mu.weight"] + dlat[:, D:2 * D] @ sd["emotion_log_var.weight"]
    want_c = dlat[:, 2 * D:3 * D] @ sd["cause_mu.weight"] + dlat[:, 3 * D:] @ sd["cause_log_var.weight"]
    assert relnorm(d_in[0], want_e) <= 1e-5 and relnorm(d_in[1], want_c) <= 1e-5
    # the pooler is unused: exactly zero gradient; the adapters keep .grad None
    assert float(model.encoder.pooler.dense.weight.grad.abs().max()) == 0.0
    assert model.emotion_adapter.in_proj_weight.grad is None


@pytest.mark.parametrize("mode", ["entmax", "raw"])
def test_dense_is_forced_and_results_repeat(mode):
    B, S = 8, 128
    b = _batch(B, S)
    runs = []
    for varlen, cls_only in ((True, True), (False, False), (True, True)):
        model = _model(mode)
        model.varlen, model.cls_only_last = varlen, cls_only
        model.set_noise(*_noise())
        loss = model(*_call(b))
        loss.backward()
        assert model._last_call.pack is None and model._last_call.cls is None
        runs.append((loss.detach().clone(), model._flat_grad.clone()))
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])


def test_no_adapter_is_bitwise_todays_model():
    b = _batch(8, 128)
    res = []
    for kw in ({}, dict(adapter="false")):
        opt = M.make_opt(pair_bow_dim=257, dropout=0.0, **kw)
        assert hasattr(opt, "adapter") == bool(kw)
        model = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=1000, layers=2, hidden_dropout=0.0, attn_dropout=0.0), seed=3)
        model.to("cuda").train()
        model.set_noise(*_noise())
        loss = model(*_call(b))
        loss.backward()
        res.append((loss.detach().clone(), model._flat_grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("mode", ["entmax", "sparsemax", "raw"])
def test_three_adam_steps_leave_the_frozen_tensors_alone(mode):
    b = _batch(8, 128)
    frozen = ("encoder.pooler.dense.weight", "encoder.pooler.dense.bias", "emotion_mu.weight", "cause_log_var.bias")
    trajs = []
    for fused in (True, False):
        model = _model(mode)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        q0 = (model.emotion_q.clone(), model.cause_q.clone())
        opt = M.FusedAdam(model, lr=1e-5) if fused else torch.optim.Adam(model.get_params(), lr=1e-5)
        for it in range(3):
            opt.zero_grad()
            model.set_noise(*_noise(seed=it))
            model(*_call(b, it)).backward()
            opt.step()
        torch.cuda.synchronize()
        after = model.state_dict()
        for k in list(frozen) + model._adapter_names:
            assert torch.equal(after[k], before[k]), k
        assert torch.equal(model.emotion_q, q0[0]) and torch.equal(model.cause_q, q0[1])
        assert not torch.equal(after["decoder.weight"], before["decoder.weight"])
        trajs.append({k: v.detach().clone() for k, v in after.items()})
    for k in trajs[0]:              # the bound smoke() holds the fused step to against the fp32 oracle
        if k.endswith("attention.self.key.bias"):
            continue                # its exact gradient is 0 (softmax is shift-invariant): Adam turns the rounding noise into +-lr steps
        d = (trajs[0][k] - trajs[1][k]).abs()
        assert float(d.max()) <= 2.02e-5 and float((d <= 2e-6).float().mean()) >= 0.90, (k, float(d.max()))


@pytest.mark.parametrize("mode", ["sparsemax", "raw"])
def test_pair_probabilities_use_the_adapters(mode):
    model = _model(mode).eval()
    b = _batch(16, 128)
    eps = _noise()
    model.set_noise(*eps)
    out = model.forward_terms(*_call(b))
    Wp = model.pair_classifier.weight.detach()
    want = torch.sigmoid(out["z"] @ Wp.T + model.pair_classifier.bias.detach()).reshape(-1)
    model.set_noise(*eps)
    got = model.pair_probabilities(b["input_ids"], b["attention_masks"], b["token_type_ids"])     # one chunk: the same encoder launch shapes
    assert float((got - want).abs().max()) <= 1e-6
    preds = model.get_pair_preds(b["input_ids"], b["attention_masks"], b["token_type_ids"])
    assert len(preds) == 16
    chunked = model.pair_probabilities(b["input_ids"], b["attention_masks"], b["token_type_ids"], chunk=8)   # fresh noise, same shapes
    assert chunked.shape == got.shape and bool(((chunked > 0) & (chunked < 1)).all())


def test_checkpoint_round_trip_in_adapter_mode(tmp_path):
    b = _batch(8, 128)
    m1 = _model("entmax", seed=5)
    T.save_ckp(m1.state_dict(), str(tmp_path), "adapter")
    m2 = _model("entmax", seed=9)
    T.load_ckp(str(tmp_path / "adapter.pt"), m2)
    m2.emotion_q, m2.cause_q = m1.emotion_q.clone(), m1.cause_q.clone()    # non-persistent: the caller carries them
    res = []
    for m in (m1, m2):
        m.set_noise(*_noise())
        res.append(m.forward_terms(*_call(b)))
    for k in ("loss", "mu_e", "lv_c", "adapter_e"):
        assert torch.equal(res[0][k], res[1][k]), k


def test_a_weight_written_through_data_takes_effect():
    """u is rebuilt on every call: a write that bypasses the version counter (.data) is seen by the next forward."""
    model = _model("sparsemax")
    b = _batch(8, 128)
    model.set_noise(*_noise())
    first = model.forward_terms(*_call(b))["adapter_e"]
    model.emotion_adapter.k_proj.weight.data.mul_(3.0)
    model.emotion_q.data.mul_(-1.0)
    model.debug_fp32 = True
    model.set_noise(*_noise())
    out = model.forward_terms(*_call(b))
    x = model._ws[("f32", 8, 128)].x.double().cpu().reshape(8, 128, H)
    a_e, _ = _adapter_ref(model, x)
    assert not torch.equal(out["adapter_e"], first)
    assert relnorm(out["adapter_e"], a_e) <= 1e-5
