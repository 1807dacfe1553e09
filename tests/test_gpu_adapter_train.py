"""opt.train_adapter: the sentence adapters' weight gradients (carel_adapter_backward_weights, csrc/adapter.hip) against fp64 autograd of
the reference's own computation (tests/adapter_restate.py) with the weights as leaves, and their wiring into DrlClassifier: flat
layout, FusedAdam / torch.optim.Adam, checkpoints.  Helpers are those of tests/test_gpu_adapter.py."""
import ctypes as C
import math

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import ops
from carel_vae_amd import training as T
from tests import adapter_restate as R
from tests import test_gpu_adapter as A

pytestmark = pytest.mark.gpu

H = A.H
relnorm = A.relnorm
DESTS = ("d_q_w", "d_q_b", "d_k_w", "d_k_b", "d_v_w", "d_v_b", "d_o_w", "d_o_b")


# Seeds.  tests/test_gpu_adapter.py's _inputs puts a tied and a constant sample into every batch of three or more, and at kscale 40 the
# remaining samples of a small batch can all have one-token supports: the q / k gradients are then exactly zero but for the tied and the
# constant sample's, which are zero by cancellation -- a relative norm would compare rounding noise with zero.  A case whose default
# seed gives such a side takes the first salt that does not; the criterion (conditioned(), on the fp64 reference alone, so the same on
# every machine) is asserted by the test.
SALT = {("entmax", 128, 7, 40): 5, ("sparsemax", 32, 7, 40): 11, ("sparsemax", 96, 7, 40): 10, ("sparsemax", 128, 7, 40): 29}


def conditioned(ref, d_out):
    """Every q / k gradient of the fp64 reference carries signal: its norm is at least 1e-6 of ||d_out|| (well-posed sides measure
    1.7e-3 of it and more, cancelled ones below 1e-11), or, for a single sample with a one-token support, it is exactly zero (the kernels
    must then give exact zeros too)."""
    B = d_out.shape[1]
    return all(float(ref[side][k].norm()) >= 1e-6 * float(d_out[side].norm()) or (B == 1 and float(ref[side][k].norm()) == 0.0)
               for side in range(2) for k in ("d_q_w", "d_q_b", "d_k_w"))


# Cases that cannot meet 1e-4 in float32 get four times the float32 restatement's own error, computed by the test.  None is left:
# ("raw", 4, 96, 1, 40) -- a single sample whose four softmax rows are nearly one-hot, so that p (dp - sum p dp) of the dominant token is
# a difference of nearly equal numbers -- measured 8.2e-4 (d_q_w, d_q_b) and 7.9e-4 (d_k_w) for the kernels AND for the float32
# restatement while the kernels evaluated that expression as written.  They now shift dp by its value at the largest p
# (softmax_backward, csrc/adapter.hip) and measure 6.4e-7 / 5.6e-7 on that case on an MI355X; the restatement is still at 8.2e-4.
F32_LIMITED = set()


def f32_error(r64, r32):
    """{(side, dest): error of the float32 restatement against its float64 self}"""
    return {(side, k): relnorm(r32[side][k], v) for side in range(2) for k, v in r64[side].items() if k != "d_k_b"}


def sweep_case(mode, G, S, B, kscale):
    """Inputs of one sweep case (CPU; weights and hidden states f32-representable fp64).
    d_out rows of samples whose sparsemax scores sit within 1e-3 of the support threshold are zeroed (that backward is discontinuous
    there): such a sample contributes exactly nothing on either side.  -> (ws, qs, Hs, d_out, kept samples per side)."""
    g = torch.Generator().manual_seed(1000 * S + 10 * B + int(kscale) + 7919 * SALT.get((mode, S, B, int(kscale)), 0))
    ws = [A._weights(mode, g, kscale) for _ in range(2)]
    qs = [torch.randn(H, generator=g).double() for _ in range(2)]
    Hs = A._inputs(B, S, seed=3 * S + B)
    d_out = torch.randn(2, B, H, generator=g).double()
    kept = []
    for side in range(2):
        keep = torch.ones(B, dtype=torch.bool)
        if mode == "sparsemax":
            with torch.no_grad():
                qp = qs[side] @ ws[side]["q_proj.weight"].T + ws[side]["q_proj.bias"]
                sc = (Hs @ ws[side]["k_proj.weight"].T + ws[side]["k_proj.bias"]) @ qp / math.sqrt(H)
            keep = A._margin_ok(sc, mode)
            d_out[side][~keep] = 0.0
        kept.append(int(keep.sum()))
    return ws, qs, Hs, d_out, kept


def reference_grads(mode, G, ws, qs, Hs, d_out, dtype=torch.float64):
    """Autograd of the restatement in `dtype` with the weights as leaves -> per side, a dict keyed like the C call's destinations."""
    out = []
    for side in range(2):
        leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in ws[side].items()}
        o, _ = R.adapter_out(Hs.to(dtype), qs[side].to(dtype), leaves, mode, G)
        (o * d_out[side].to(dtype)).sum().backward()
        gr = {k: v.grad.double() for k, v in leaves.items()}
        if mode == "raw":
            wi, bi = gr["in_proj_weight"], gr["in_proj_bias"]
            out.append(dict(d_q_w=wi[:H], d_q_b=bi[:H], d_k_w=wi[H:2 * H], d_k_b=bi[H:2 * H], d_v_w=wi[2 * H:], d_v_b=bi[2 * H:],
                            d_o_w=gr["out_proj.weight"], d_o_b=gr["out_proj.bias"]))
        else:
            out.append(dict(d_q_w=gr["q_proj.weight"], d_q_b=gr["q_proj.bias"], d_k_w=gr["k_proj.weight"], d_k_b=gr["k_proj.bias"]))
    return out


def _dests():
    """Destinations laid out as the model's are: raw mode's q / k / v blocks are slices of one in_proj gradient.  All NaN."""
    nan = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=torch.float32)      # noqa: E731
    out = []
    for _ in range(2):
        wi, bi = nan(3 * H, H), nan(3 * H)
        out.append(dict(d_q_w=wi[:H], d_q_b=bi[:H], d_k_w=wi[H:2 * H], d_k_b=bi[H:2 * H], d_v_w=wi[2 * H:], d_v_b=bi[2 * H:],
                        d_o_w=nan(H, H), d_o_b=nan(H)))
    return out


def _snapshot(dests):
    return [{k: v.clone() for k, v in d.items()} for d in dests]


@pytest.mark.parametrize("mode,G", A.MODES)
@pytest.mark.parametrize("S", [32, 96, 128])
@pytest.mark.parametrize("B", [1, 7, 33])
@pytest.mark.parametrize("kscale", [1.0, 40.0])
def test_weight_gradients_vs_float64_autograd(mode, G, S, B, kscale):
    ws, qs, Hs, d_out, kept = sweep_case(mode, G, S, B, kscale)
    assert min(kept) >= (B + 1) // 2, kept                   # at least half the samples remain on each side
    ref = reference_grads(mode, G, ws, qs, Hs, d_out)
    assert conditioned(ref, d_out)                           # the inputs carry signal (see SALT)
    e32 = None
    if (mode, G, S, B, int(kscale)) in F32_LIMITED:
        e32 = f32_error(ref, reference_grads(mode, G, ws, qs, Hs, d_out, dtype=torch.float32))
    Bp = B + 1
    out0, dx0 = A._run_kernels(mode, G, Hs, Bp, qs, ws, d_out)          # a run without the new call
    x = torch.zeros((Bp * S, H), device="cuda", dtype=torch.float32)
    x[:B * S] = Hs.reshape(B * S, H).float().cuda()
    buf = ops.AdapterBuffers(B, S, G, x.device)
    u = torch.empty((2, G, H), device="cuda", dtype=torch.float32)
    dx = torch.full((Bp * S, H), float("nan"), device="cuda", dtype=torch.float32)
    qd = [q.float().cuda().contiguous() for q in qs]
    a = ops.adapter_args(mode, G, qd, [A._kernel_weights(w, mode) for w in ws], u, buf, Bp, x=x, dx=dx)
    ops.adapter_build_u(a)
    ops.adapter_forward(a)
    buf.d_out.copy_(d_out.float())
    ops.adapter_backward(a)
    dests = _dests()
    ops.adapter_backward_weights(a, ops.adapter_wgrad_args(buf, dests))
    first = _snapshot(dests)
    ops.adapter_backward_weights(a, ops.adapter_wgrad_args(buf, dests))
    second = _snapshot(dests)
    ops.adapter_backward_weights(a, ops.adapter_wgrad_args(buf, dests, accumulate=True))
    torch.cuda.synchronize()
    assert torch.equal(buf.out, out0) and torch.equal(dx, dx0), "the new call must leave out and dx alone"
    written = DESTS if mode == "raw" else DESTS[:4]
    for side in range(2):
        for k in DESTS:
            f, s, acc = first[side][k], second[side][k], dests[side][k]
            if k not in written:                             # tensors the forward never reads: untouched
                assert bool(torch.isnan(f).all()) and bool(torch.isnan(acc).all()), k
                continue
            assert bool(torch.isfinite(f).all()), k
            assert torch.equal(f, s), "repeat call not bitwise identical: " + k
            assert torch.equal(acc, f + f), "accumulate = 1 must give first + first: " + k
            if k == "d_k_b":
                assert float(f.abs().max()) == 0.0           # exactly zero: the normalisers are translation-invariant
                continue
            # 1e-4, the bound the adapter backward test holds dx to (F32_LIMITED: four times the float32 restatement's own error)
            e, bound = relnorm(f, ref[side][k]), 1e-4
            if e32 is not None and k in ("d_q_w", "d_q_b", "d_k_w"):
                bound = max(bound, 4 * e32[(side, k)])
                print("WGRAD f32 restatement %s side %d: %.3g" % (k, side, e32[(side, k)]))
            print("WGRAD %s G%d S%d B%d k%d side %d %s: %.3g (bound %.3g)" % (mode, G, S, B, kscale, side, k, e, bound))
            assert e <= bound, (side, k, e, bound)


def test_argument_errors_are_refused_before_any_launch():
    B, S, G = 2, 32, 1
    buf = ops.AdapterBuffers(B, S, G, torch.device("cuda"))
    x = torch.zeros((B * S, H), device="cuda")
    u = torch.zeros((2, G, H), device="cuda")
    g = torch.Generator().manual_seed(0)
    ws = [A._kernel_weights(A._weights("entmax", g, 1.0), "entmax") for _ in range(2)]
    qd = [torch.zeros(H, device="cuda") for _ in range(2)]
    a = ops.adapter_args("entmax", G, qd, ws, u, buf, B, x=x)
    dests = _dests()
    gw = ops.adapter_wgrad_args(buf, dests)
    gw.accumulate = 2
    with pytest.raises(L.CarelError, match="accumulate"):
        ops.adapter_backward_weights(a, gw)
    gw = ops.adapter_wgrad_args(buf, dests)
    gw.d_k_b[1] = None
    with pytest.raises(L.CarelError, match="d_k"):
        ops.adapter_backward_weights(a, gw)
    a.seq_len = 160                                          # widens nothing: the lengths ad_check accepts
    with pytest.raises(L.CarelError, match="seq_len"):
        ops.adapter_backward_weights(a, ops.adapter_wgrad_args(buf, dests))
    a.seq_len, a.mode = S, 0                                 # raw needs d_v_* / d_o_*
    gw = ops.adapter_wgrad_args(buf, [{k: v for k, v in d.items() if k in DESTS[:4]} for d in dests])
    with pytest.raises(L.CarelError, match="raw"):
        ops.adapter_backward_weights(a, gw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for d in dests for v in d.values())


# ---------------------------------------------------------------------------------------------- the model
SHAPES = [(8, 128), (7, 96)]
LATENT = [n + t for n in ("emotion_mu", "emotion_log_var", "cause_mu", "cause_log_var") for t in (".weight", ".bias")]


def _step(model, b, it=3, seed=0):
    model.set_noise(*A._noise(seed=seed))
    loss = model(*A._call(b, it))
    loss.backward()
    return loss.detach().clone()


@pytest.mark.parametrize("mode", ["entmax", "sparsemax", "raw"])
@pytest.mark.parametrize("B,S", SHAPES)
def test_training_the_adapters_leaves_every_other_bit_alone(mode, B, S):
    b = A._batch(B, S)
    frozen, trained = A._model(mode), A._model(mode, train_adapter=True)
    lf, lt = _step(frozen, b), _step(trained, b)
    assert torch.equal(lf, lt)
    for k in frozen._order:
        if "_adapter." in k:
            continue
        assert torch.equal(frozen._grad_view(k), trained._grad_view(k)), k
        assert frozen._named[k].grad is not None and trained._named[k].grad is not None
    for k in trained._adapter_names:
        assert frozen._named[k].grad is None
        assert (trained._named[k].grad is not None) == (k in trained._adapter_train_names), k
    assert len(trained._adapter_train_names) == 8


@pytest.mark.parametrize("mode,heads", [("entmax", 4), ("sparsemax", 4), ("raw", 4)])
@pytest.mark.parametrize("B,S", SHAPES)
def test_model_adapter_gradients_vs_float64_autograd(mode, heads, B, S):
    """The adapters' .grad against fp64 autograd of the restatement, given the model's own last hidden states and the tail's d head_in."""
    model = A._model(mode, heads, train_adapter="true")
    b = A._batch(B, S)
    Bp = model._padded_batch(B, S)
    model.set_noise(*A._noise())
    loss = model(*A._call(b))
    c = model._last_call
    x = A._copy_dev(L.load().carel_encoder_x_last(C.byref(c.ea)), Bp * S * H).view(Bp, S, H)[:B].double().cpu()
    loss.backward()
    d_in = model._ws[("adapter", B, S)].d_out.double().cpu()
    sd = model.state_dict()
    for i, side in enumerate(("emotion", "cause")):
        leaves = {k: v.clone().requires_grad_() for k, v in R.adapter_weights(sd, side).items()}
        q = getattr(model, side + "_q").double().cpu().reshape(-1)
        o, _ = R.adapter_out(x, q, leaves, mode, model.head_number)
        (o * d_in[i]).sum().backward()
        for n in M.ADAPTER_TRAINED[mode]:
            got = model._named["%s_adapter.%s" % (side, n)].grad
            want = leaves[n].grad
            if n == "k_proj.bias":
                assert float(got.abs().max()) == 0.0
                continue
            if n == "in_proj_bias":
                assert float(got[H:2 * H].abs().max()) == 0.0
            e = relnorm(got, want)
            print("%s %s.%s: %.3g" % (mode, side, n, e))
            assert e <= 1e-4, (side, n, e)
        for n in leaves:
            if n not in M.ADAPTER_TRAINED[mode]:
                assert model._named["%s_adapter.%s" % (side, n)].grad is None and leaves[n].grad is None, n


@pytest.mark.parametrize("mode", ["entmax", "sparsemax", "raw"])
def test_three_adam_steps_train_the_adapters(mode):
    b = A._batch(8, 128)
    trajs, firsts = [], []
    for fused in (True, False):
        model = A._model(mode, train_adapter=True)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        q0 = (model.emotion_q.clone(), model.cause_q.clone())
        model.set_noise(*A._noise())
        first = model.forward_terms(*A._call(b))["adapter_e"]
        opt = M.FusedAdam(model, lr=1e-5) if fused else torch.optim.Adam(model.get_params(), lr=1e-5)
        for it in range(3):
            opt.zero_grad()
            model.set_noise(*A._noise(seed=it))
            model(*A._call(b, it)).backward()
            opt.step()
        torch.cuda.synchronize()
        after = model.state_dict()
        trained = model._adapter_train_names
        for k in trained:
            if k.endswith("k_proj.bias"):
                assert torch.equal(after[k], before[k]), k            # zero gradient: Adam leaves it where it is
            else:
                assert not torch.equal(after[k], before[k]), k
        for k in [k for k in model._adapter_names if k not in trained] + LATENT + ["encoder.pooler.dense.weight", "encoder.pooler.dense.bias"]:
            assert torch.equal(after[k], before[k]), k
        assert torch.equal(model.emotion_q, q0[0]) and torch.equal(model.cause_q, q0[1])
        assert not torch.equal(after["decoder.weight"], before["decoder.weight"])
        model.set_noise(*A._noise())
        assert not torch.equal(model.forward_terms(*A._call(b))["adapter_e"], first)
        trajs.append({k: v.detach().clone() for k, v in after.items()})
    for k in trajs[0]:              # the bounds of test_three_adam_steps_leave_the_frozen_tensors_alone
        if k.endswith("attention.self.key.bias"):
            continue
        d = (trajs[0][k] - trajs[1][k]).abs()
        assert float(d.max()) <= 2.02e-5 and float((d <= 2e-6).float().mean()) >= 0.90, (k, float(d.max()))


def test_train_adapter_false_is_bitwise_the_model_without_the_keyword():
    b = A._batch(8, 128)
    res = []
    for kw in ({}, dict(train_adapter=False), dict(train_adapter="false")):
        model = A._model("entmax", **kw)
        loss = _step(model, b)
        res.append((loss, model._flat_grad.clone(), dict(model._offs)))
        for k in model._adapter_names:
            assert model._named[k].grad is None, k
    for r in res[1:]:
        assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1]) and r[2] == res[0][2]


def test_checkpoint_round_trip_after_a_trained_step(tmp_path):
    b = A._batch(8, 128)
    m1 = A._model("entmax", seed=5, train_adapter=True)
    opt = M.FusedAdam(m1, lr=1e-5)
    opt.zero_grad()
    _step(m1, b)
    opt.step()
    T.save_ckp(m1.state_dict(), str(tmp_path), "adapter_trained")
    m2 = A._model("entmax", seed=9, train_adapter=True)
    T.load_ckp(str(tmp_path / "adapter_trained.pt"), m2)
    m2.emotion_q, m2.cause_q = m1.emotion_q.clone(), m1.cause_q.clone()    # non-persistent: the caller carries them
    res = []
    for m in (m1, m2):
        m.set_noise(*A._noise())
        res.append(m.forward_terms(*A._call(b)))
    for k in ("loss", "mu_e", "lv_c", "adapter_e", "adapter_c"):
        assert torch.equal(res[0][k], res[1][k]), k
