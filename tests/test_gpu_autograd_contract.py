"""The autograd contract of the whole-step functions ("autograd contract"): what `backward()` does with an upstream
gradient other than 1, with parameters that already hold a gradient, and with a gradient on the sampled embeddings -- the
hand-written glue between "the kernels wrote gradients for grad_output = 1 into the flat buffer" and torch's semantics
(_TrainLoss / _GanLosses / _AprxLoss, _run_backward / _run_backward_gan / _overwriting_grads, _EnLosses / _run_backward_en, _EmbedFn /
_backward; under them carel_tail_backward_dz, carel_scale_f32, carel_axpy_f32).

Front ends (the smallest configurations the suite has, two encoder layers, B <= 16, S <= 64): DrlClassifier in mmd mode on the dense
golden case and on the ragged one (packed), in vi mode, in gan mode; the three-space DrlClassifierEn with its seven losses;
SentenceTransformer (BERT and MPNet geometry) through _EmbedFn with an upstream g [B, 768].  Noise, iteration and the dropout seed
(the forward counter) are pinned per call, so repeated forwards are the same function.

  (a) control     two runs from .grad = None give identical bits for every parameter (the precondition of b and d)
  (b) 2^k scale   (k * loss).backward() == k * grad_1 exactly, one loss at a time; a loss reaches its own parameters only
  (c) 0.37 scale  against 0.37 x the oracle's gradients, with the oracle and the constants of that front end's own gradient test
  (d) accumulate  a second backward without clearing; after zero_grad(set_to_none=False); a half-cleared adversary; the approximation
                  network's gradients under an accumulating vae backward; the dead pair head under strict_pair_skip
  (e) grad_z      a loss on the sampled embeddings alone: tail gradients against float64, the encoder's by linearity, heads exactly 0
  (f) fused Adam  micro-batches accumulate without the fused update firing; one step() then equals the plain optimiser's

Every comparison is exact or uses a named constant of the test it follows."""
import functools

import numpy as np
import pytest
import torch

from carel_vae_amd import drl_classifier as M
from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from oracle import carel_oracle_st as ST
from tests import gan_restate as R
from tests import test_gpu_en_adv as TE
from tests import test_gpu_gan_model as TG
from tests import test_gpu_model as TM
from tests import test_gpu_tail_sweep as TS
from tests import test_gpu_triplet as TT
from tests import test_gpu_vi as TV
from tests.tail_restate import TAIL_KEYS

pytestmark = pytest.mark.gpu
relnorm = TM.relnorm


# ------------------------------------------------------------------------------------------------ front ends
class Front:
    """One model with pinned inputs.  names: the losses forward() returns; sequence(): the backward calls of the reference's loop, in
    its order, each loss times scales[i] (None: that call is left out) and with no zero_grad between them; owns(i, key): may a
    backward of loss i ALONE write parameter `key`."""

    names = ("loss",)

    def params(self):
        return dict(self.model.named_parameters())

    def sequence(self, losses, scales):
        live = [i for i, s in enumerate(scales) if s is not None]
        for i in live:
            (scales[i] * losses[i]).backward(retain_graph=i != live[-1])

    def owns(self, i, key):
        return True

    def one_logit(self, key, g):
        return False


def _check_fp32_oracle(got, grads, k, one_logit=lambda key, g: False):
    """tests/test_gpu_model.py::test_gradients_vs_oracle with the oracle's gradients times k; a one-logit bias (one_logit(key, g)) by
    the rule and constants of tests/test_gpu_en_adv.py, its absolute part times |k| as well."""
    worst = {}
    for key, g in grads.items():
        assert got[key] is not None, key
        if g is None or float(g.norm()) < 1e-7:      # key bias: analytically zero (softmax shift invariance)
            qb = got[key.replace("key", "query")]
            assert float(got[key].norm()) < 0.05 * float(qb.norm()) + 1e-4 * abs(k), key
            continue
        if one_logit(key, g):
            rel, ab = TE.TOL_ONE_LOGIT_BIAS
            assert abs(float(got[key]) - k * float(g)) <= rel * abs(k * float(g)) + abs(k) * ab, (key, float(got[key]), k * float(g))
            continue
        worst[key] = relnorm(got[key], k * g)
    print("worst", sorted(worst.items(), key=lambda kv: -kv[1])[:3], "median", float(np.median(list(worst.values()))))
    bad = {key: v for key, v in worst.items() if v > TM.TOL_GRAD_FP32_WORST}
    assert not bad, bad
    assert np.median(list(worst.values())) < TM.TOL_GRAD_FP32_MEDIAN


class Mmd(Front):
    def __init__(self, golden_dir, name, packed):
        self.cfg, self.opt = TM.CASES[name]
        self.z, self.batch = TM.load(golden_dir, name)
        wseed, self.it = int(self.z["meta"][5]), int(self.z["meta"][8])
        self.model, self.P = TM.build(self.cfg, self.opt, wseed)
        self.model.train()
        self.model.varlen = packed
        self.packed = packed
        self.eps = torch.from_numpy(self.z["eps_e_0"]), torch.from_numpy(self.z["eps_c_0"])

    def forward(self, batch=None):
        m = self.model
        m.set_noise(*self.eps)
        m._fwd_count = 0
        loss = m(*TM.call(m, self.batch if batch is None else batch, self.it))
        assert (m._last_call.pack is not None) == self.packed
        return (loss,)

    @functools.lru_cache(None)
    def oracle(self):
        return O.loss_and_grads(self.P, self.batch, self.it, self.cfg, self.opt, *self.eps)[1]

    def check_oracle(self, got, k):
        _check_fp32_oracle(got, self.oracle(), k)


class Vi(Front):
    names = ("aprx", "vae")

    def __init__(self, golden_dir):
        self.cfg, self.opt, self.z, self.batch, self.model, self.P = TV._build(golden_dir)
        self.model.train()
        self.eps = torch.from_numpy(self.z["eps_e_0"]), torch.from_numpy(self.z["eps_c_0"])

    def forward(self):
        m = self.model
        m.set_noise(*self.eps)
        m._fwd_count = 0
        b = {k: v.cuda() for k, v in self.batch.items()}
        out = m(b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], 5)
        return out[2], out[3]

    def owns(self, i, key):
        return (key in O.VI_KEYS) == (i == 0)

    def one_logit(self, key, g):
        return g.numel() == 1

    def check_oracle(self, got, k):
        """The vae loss is the `none` model's with the one-logit emotion head (what O.vi_train_step differentiates); the approximation
        network's eight gradients against k times the oracle's on the device's own z, as tests/test_gpu_vi.py::test_vi_kernels_vs_oracle."""
        D = self.opt.ec_dim
        z = self.model._last_call.buf.z.detach().cpu()
        leaf = {key: self.P[key].clone().requires_grad_(True) for key in O.VI_KEYS}
        O.vi_aprx_loss(leaf, z[:, :D], z[:, D:]).backward()
        for key in O.VI_KEYS:
            r = k * leaf[key].grad
            assert float((got[key].cpu() - r).abs().max()) <= TV.TOL_APRX_GRAD * max(float(r.abs().max()), 1e-3 * abs(k)), key
        grads = O.loss_and_grads(self.P, self.batch, 5, self.cfg, self.opt, *self.eps, disentangle="none", emotion_head="bce")[1]
        _check_fp32_oracle(got, {key: g for key, g in grads.items() if key not in O.VI_KEYS}, k, self.one_logit)


class Gan(Front):
    names = R.LOSS_NAMES

    def __init__(self, golden_dir):
        self.opt = R.gan_opt(pair_bow_dim=211, dropout=0.0)
        self.z, self.batch = TG.load(golden_dir)
        self.model, self.P = TG.build(self.opt, int(self.z["meta"][5]))
        self.model.train()
        self.eps = torch.from_numpy(self.z["eps_e_0"]), torch.from_numpy(self.z["eps_c_0"])

    def forward(self):
        m = self.model
        m.set_noise(*self.eps)
        m._fwd_count = 0
        return m(*TG.call(self.batch, 7))

    def owns(self, i, key):
        return i == 2 or key.startswith(TG.DISC[i] + ".")

    def one_logit(self, key, g):
        return g.numel() == 1

    def check_oracle(self, got, k):
        """The restatement of tests/gan_restate.py in fp32; the adversaries at the constants of test_three_steps_follow_the_reference
        (those of tests/test_gpu_en_adv.py), everything else as the two-space model."""
        grads = R.loss_and_grads(self.P, self.batch, 7, TG.CFG, self.opt, *self.eps)[1]
        for key in R.GAN_KEYS:
            if key.endswith("weight"):
                assert relnorm(got[key], k * grads[key]) <= TE.TOL_GRAD_HEADS, key
        _check_fp32_oracle(got, {key: g for key, g in grads.items() if not (key in R.GAN_KEYS and key.endswith("weight"))}, k, self.one_logit)


class En(Front):
    names = OE.LOSS_NAMES
    GROUP = ("content_disc", "content_disc", "emotion_disc", "ec_disc", "cause_disc", "ce_disc")

    def __init__(self, golden_dir):
        self.opt = OE.OptEn(pair_bow_dim=211, dropout=0.0)
        self.z, self.batch = TE.load(golden_dir)
        self.model, self.P = TE.build(self.opt, int(self.z["meta"][5]))
        self.model.train()
        self.eps = TE.eps_of(self.z, 0)

    def forward(self):
        m = self.model
        m.set_noise(self.eps["con"], self.eps["e"], self.eps["c"])
        m._fwd_count = 0
        return m(*TE.call(self.batch, 7))

    def sequence(self, losses, scales):
        """tests/test_gpu_en_adv.py::reference_step without its zero_grad calls: the two content-discriminator losses go back as one sum."""
        calls = []
        if scales[0] is not None and scales[1] is not None:
            calls.append(scales[0] * losses[0] + scales[1] * losses[1])
        else:
            calls += [scales[i] * losses[i] for i in (0, 1) if scales[i] is not None]
        calls += [scales[i] * losses[i] for i in range(2, 7) if scales[i] is not None]
        for j, c in enumerate(calls):
            c.backward(retain_graph=j != len(calls) - 1)

    def owns(self, i, key):
        if key.startswith(tuple(h + "." for h in OE.LATENT_HEADS)):          # in no optimiser group: no gradient is produced
            return False
        return i == 6 or key.startswith(self.GROUP[i] + ".")

    def check_oracle(self, got, k):
        """tests/test_gpu_en_adv.py::test_terms_and_gradients_vs_oracle_and_golden with the oracle's gradients times k."""
        grads = OE.loss_and_grads(self.P, self.batch, 7, TE.CFG, self.opt, self.eps, quant=O.bf16_round)[1]
        worst = {}
        for key, g in grads.items():
            assert got[key] is not None, key
            if float(g.norm()) < 1e-7 or key.endswith("key.bias"):
                continue
            if g.numel() == 1:
                rel, ab = TE.TOL_ONE_LOGIT_BIAS
                assert abs(float(got[key]) - k * float(g)) <= rel * abs(k * float(g)) + abs(k) * ab, (key, float(got[key]), k * float(g))
                continue
            worst[key] = relnorm(got[key], k * g)
        bad = {key: v for key, v in worst.items() if v > (TE.TOL_GRAD_HEADS if not key.startswith("encoder.") else TE.TOL_GRAD_ENCODER)}
        assert not bad, bad
        for h in OE.LATENT_HEADS:
            assert got[h + ".weight"] is None


class Sent(Front):
    names = ("embedding",)

    def __init__(self, variant):
        self.cfg, self.P, self.model, sents, _ = TT._setup(variant=variant)
        self.model.train(True)
        self.feats = self.model.tokenize(sents[:8])
        self.g = torch.randn((8, 768), generator=torch.Generator().manual_seed(8))

    def forward(self):
        self.model._fwd = 0
        emb = self.model(self.feats)["sentence_embedding"]
        return ((emb * self.g.cuda()).sum(),)            # backward hands _EmbedFn the upstream gradient scale * g

    def check_oracle(self, got, k):
        """tests/test_gpu_triplet.py::test_first_step_gradients_and_clip_norm_against_the_restatement for the upstream gradient k g."""
        keys = ST.encoder_keys(self.P)
        Wr = {key: (v.clone().requires_grad_(True) if key in keys else v) for key, v in self.P.items()}
        f = self.feats
        (ST.encode(Wr, f["input_ids"], f["attention_mask"], f["token_type_ids"], self.cfg) * (k * self.g)).sum().backward()
        worst = {}
        for key in keys:
            gr = Wr[key].grad
            if gr is None or float(gr.norm()) < 1e-7 or key.endswith("key.bias"):     # (key bias: analytically zero, rounding noise in both)
                continue
            worst[key] = relnorm(got[TT._public(self.model, key)], gr)
        assert max(worst.values()) < TT.TOL_GRAD_WORST and float(np.median(list(worst.values()))) < TT.TOL_GRAD_MEDIAN, \
            sorted(worst.items(), key=lambda kv: -kv[1])[:3]


FRONTS = ("mmd_dense", "mmd_packed", "vi", "gan", "en", "st_bert", "st_mpnet")
MULTI = ("vi", "gan", "en")


@functools.lru_cache(None)
def front(name, golden_dir):
    if name == "mmd_dense":
        return Mmd(golden_dir, "zh_small", packed=False)
    if name == "mmd_packed":
        return Mmd(golden_dir, "zh_ragged", packed=True)
    if name in ("st_bert", "st_mpnet"):
        return Sent(name[3:])
    return {"vi": Vi, "gan": Gan, "en": En}[name](golden_dir)


# ------------------------------------------------------------------------------------------------ runs
def clear(f):
    for p in f.params().values():
        p.grad = None


def snapshot(f):
    torch.cuda.synchronize()
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in f.params().items()}


def run(f, scales=None, keep_grads=False):
    """One forward and the backward sequence; from .grad = None unless keep_grads.  -> {key: gradient or None}."""
    if not keep_grads:
        clear(f)
    f.sequence(f.forward(), [1.0] * len(f.names) if scales is None else scales)
    return snapshot(f)


def only(f, i, s=1.0):
    return [s if j == i else None for j in range(len(f.names))]


def assert_same(got, want, what):
    for k, w in want.items():
        assert (got[k] is None) == (w is None), (what, k, "None-ness differs")
        if w is not None:
            assert torch.equal(got[k], w), (what, k, float((got[k] - w).abs().max()), float(w.abs().max()))


# ------------------------------------------------------------------------------------------------ (a) control
@pytest.mark.parametrize("name", FRONTS)
def test_two_runs_give_the_same_bits(golden_dir, name):
    f = front(name, golden_dir)
    first, second = run(f), run(f)
    assert sum(g is not None and bool(g.any()) for g in first.values()) > 0.8 * len(first)
    assert_same(second, first, "second run")


# ------------------------------------------------------------------------------------------------ (b) powers of two
@pytest.mark.parametrize("name", FRONTS)
def test_power_of_two_scale_is_exact_and_stays_in_its_group(golden_dir, name):
    """Every step of the backward is linear in the upstream gradient and a multiplication by 2^k commutes with fp32 and bf16 rounding
    (upward only, so nothing becomes denormal): any mismatch is a missed scale or a wrong range.  A loss alone writes its own
    parameters only; in the whole sequence, scaling one loss leaves every parameter outside its reach with its bits."""
    f = front(name, golden_dir)
    full = run(f)
    for i, loss in enumerate(f.names):
        base = run(f, only(f, i))
        for k, g in base.items():
            assert (g is not None) == f.owns(i, k), (loss, k, "written by a loss that does not own it" if g is not None else "not written")
        for s in (2.0, 4.0):
            got = run(f, only(f, i, s))
            assert_same(got, {k: (None if g is None else s * g) for k, g in base.items()}, "%g x %s" % (s, loss))
        if len(f.names) > 1:
            got = run(f, [2.0 if j == i else 1.0 for j in range(len(f.names))])
            assert_same({k: g for k, g in got.items() if not f.owns(i, k)}, {k: g for k, g in full.items() if not f.owns(i, k)},
                        "the sequence with 2 x %s, outside its group" % loss)


# ------------------------------------------------------------------------------------------------ (c) a scale that rounds
@pytest.mark.parametrize("name", FRONTS)
def test_general_scale_against_the_oracle(golden_dir, name):
    f = front(name, golden_dir)
    k = 0.37
    with oracle_threads():
        f.check_oracle(run(f, [k] * len(f.names)), k)


class oracle_threads:
    """`with oracle_threads():` -- torch's CPU ops (the oracle's autograd) on at most 16 threads."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(max(1, min(16, self.n)))

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


# ------------------------------------------------------------------------------------------------ (d) accumulation
# A second pass leaves ((g + a) + b) + c for an adversary's gradient g = (a + b) + c, against 2 g: a few more fp32 roundings of partial
# sums.  tests/test_gpu_gan_model.py::test_upstream_gradients_scale_each_share asserts this same property at TG.TOL_SUM_CHAIN.
def twice(f, first):
    """What a second identical sequence without zero_grad leaves, from the gradients of the first: twice the gradient (g + g is exact)
    wherever ONE call writes a parameter.  An adversary's gradient is a sum of images that separate calls add in turn -- its own
    losses', then the vae loss's entropy share -- so the second pass is that same chain of float additions continued, which is twice
    the gradient up to rounding only."""
    want = {k: (None if g is None else g + g) for k, g in first.items()}
    if len(f.names) > 1 and not isinstance(f, Vi):
        last = len(f.names) - 1
        own = [run(f, only(f, i)) for i in range(last)]
        ent = run(f, only(f, last))
        for k, g in first.items():
            writers = [own[i][k] for i in range(last) if own[i][k] is not None]
            if writers:
                acc = g
                for w in writers + [ent[k]]:
                    acc = acc + w
                want[k] = acc
    return want


@pytest.mark.parametrize("name", FRONTS)
def test_second_backward_without_clearing_accumulates(golden_dir, name):
    f = front(name, golden_dir)
    first = run(f)
    want = twice(f, first)
    run(f)
    assert_same(run(f, keep_grads=True), want, "second pass")
    for k, g in first.items():           # and the chain of additions is twice the gradient to rounding
        if g is not None:
            assert relnorm(want[k], 2.0 * g) <= TG.TOL_SUM_CHAIN, k


@pytest.mark.parametrize("name", FRONTS)
def test_backward_onto_zeroed_gradients_gives_the_fresh_bits(golden_dir, name):
    """zero_grad(set_to_none=False): the accumulate path adds what the kernels wrote to zeros."""
    f = front(name, golden_dir)
    first = run(f)
    for p in f.params().values():
        if p.grad is not None:
            p.grad.zero_()
    assert_same(run(f, keep_grads=True), first, "onto zeros")


@pytest.mark.parametrize("name,group,loss", [("gan", "ec_disc", 0), ("en", "emotion_disc", 2)])
def test_half_cleared_adversary_is_overwritten(golden_dir, name, group, loss):
    """weight.grad = None with the bias kept: the group's range is written as a whole, so it is overwritten (_group_has_grad)."""
    f = front(name, golden_dir)
    fresh = run(f, only(f, loss))
    run(f)
    f.params()[group + ".weight"].grad = None
    got = run(f, only(f, loss), keep_grads=True)
    for t in (".weight", ".bias"):
        assert torch.equal(got[group + t], fresh[group + t]), t


def test_vi_accumulating_vae_backward_leaves_the_approximation_network_alone(golden_dir):
    """The eight ec_mu / ec_log_var gradients belong to _AprxLoss.backward; the vae backward never writes them, so when it accumulates
    they must keep their bits (they were added to themselves before _run_backward kept their range out)."""
    f = front("vi", golden_dir)
    first = run(f, [None, 1.0])                          # the vae group holds a gradient
    aprx, _ = f.forward()
    aprx.backward()
    wrote = snapshot(f)
    assert all(wrote[k] is not None and bool(wrote[k].any()) for k in O.VI_KEYS)
    f.sequence(f.forward(), [None, 1.0])                 # accumulating vae backward
    got = snapshot(f)
    for k in O.VI_KEYS:
        assert torch.equal(got[k], wrote[k]), (k, relnorm(got[k], wrote[k]))
    assert_same({k: g for k, g in got.items() if k not in O.VI_KEYS}, {k: g + g for k, g in first.items() if k not in O.VI_KEYS}, "vae group")
    # and the other way round: an accumulating _AprxLoss.backward adds to its own eight only
    aprx, _ = f.forward()
    (2.0 * aprx).backward()
    again = snapshot(f)
    for k, g in got.items():
        assert torch.equal(again[k], g + 2.0 * wrote[k] if k in O.VI_KEYS else g), k


def test_strict_pair_skip_under_accumulation_keeps_the_earlier_pair_gradient(golden_dir):
    """An all-negative batch replaces the pair loss by 0.  With strict_pair_skip a backward from .grad = None leaves the pair head's
    .grad None; an accumulating one adds its zeros: the earlier gradient survives, neither doubled nor dropped."""
    f = front("mmd_dense", golden_dir)
    m = f.model
    allneg = dict(f.batch, labels=torch.zeros_like(f.batch["labels"]), cau_labels=torch.zeros_like(f.batch["cau_labels"]))
    m.strict_pair_skip = True
    try:
        first = run(f)
        (loss,) = f.forward(allneg)
        loss.backward()
        got = snapshot(f)
        clear(f)
        (loss,) = f.forward(allneg)
        loss.backward()
        alone = snapshot(f)
    finally:
        m.strict_pair_skip = False
    for k in m._pair_range_names:
        assert bool(first[k].any()) and alone[k] is None
        assert got[k] is not None and torch.equal(got[k], first[k]), k
    k = "encoder.encoder.layer.0.output.dense.weight"
    assert torch.equal(got[k], first[k] + alone[k])


# ------------------------------------------------------------------------------------------------ (e) grad_z
W_EXTRA = 0.25


def extra_loss(ze, zc):
    return W_EXTRA * ((ze * zc).sum() + ze.pow(2).mean())


def test_loss_on_the_sampled_embeddings_alone(golden_dir):
    """backward of f(z) with the returned loss unused: _TrainLoss.backward gets grad_out = None (-> 0) and grad_z.  The latent heads
    against the float64 oracle of the tail sweep on the device's own pooled rows, at that sweep's bound; the classifier and decoder
    gradients exactly 0; and for every parameter grad(loss + f) - grad(loss) = grad(f alone) at the bf16 bound of (c)."""
    f = front("mmd_dense", golden_dir)
    m, D = f.model, f.opt.ec_dim
    g_loss = run(f)
    clear(f)
    f.forward()
    extra_loss(*m.sampled_embeddings()).backward()
    g_f = snapshot(f)
    c = m._last_call
    pooled, z_dev = c.buf.pooled.detach().clone(), c.buf.z.detach().clone()
    clear(f)
    (loss,) = f.forward()
    (loss + extra_loss(*m.sampled_embeddings())).backward()
    g_both = snapshot(f)
    # the heads
    for k in TAIL_KEYS[10:]:
        assert not bool(g_f[k].any()), (k, "a loss on z alone reached a classifier / the decoder")
    zl = z_dev.clone().requires_grad_(True)
    extra_loss(zl[:, :D], zl[:, D:]).backward()
    P64 = {k: f.P[k].double().requires_grad_(True) for k in TAIL_KEYS}
    b = f.batch
    out = O.tail_forward(P64, pooled.double().cpu(), b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], f.it, f.opt,
                         f.eps[0].double(), f.eps[1].double(), train=False)
    (torch.cat((out["z_e"], out["z_c"]), dim=1) * zl.grad.double().cpu()).sum().backward()
    rep = TS.Report("grad_z")
    for k in TAIL_KEYS[2:10]:
        r = P64[k].grad
        rep.cmp(k, g_f[k], r, TS.RT_GRAD, TS.AT_GRAD * float(r.abs().max()) + 1e-9)
    rep.finish()
    # every parameter, by linearity
    worst = {}
    for k, g in g_f.items():
        if k in TAIL_KEYS[10:] or k.endswith("key.bias"):
            continue
        assert float(g.norm()) > 1e-7, k
        worst[k] = relnorm(g_both[k] - g_loss[k], g)
    ratio = float(np.median([float(g_f[k].norm()) / float(g_loss[k].norm()) for k in worst]))
    print("grad f / grad loss (median of norms) %.2f; worst %s" % (ratio, sorted(worst.items(), key=lambda kv: -kv[1])[:3]))
    bad = {k: v for k, v in worst.items() if v > TM.TOL_GRAD_FP32_WORST}
    assert not bad, bad
    assert np.median(list(worst.values())) < TM.TOL_GRAD_FP32_MEDIAN


# ------------------------------------------------------------------------------------------------ (f) fused Adam
def _fused_mmd(golden_dir):
    cfg, opt = TM.CASES["zh_small"]
    opt = O.Opt(**{**vars(opt), "dropout": 0.3})
    z, batch = TM.load(golden_dir, "zh_small")
    it = int(z["meta"][8])

    def forward(m, s):
        m.set_noise(torch.from_numpy(z[f"eps_e_{s}"]), torch.from_numpy(z[f"eps_c_{s}"]))
        return (m(*TM.call(m, batch, it + s)),)
    return (lambda: TM.build(cfg, opt, int(z["meta"][5]), train_dropout=True)[0],
            lambda m, fused: [M.FusedAdam(m, lr=1e-5, fuse_into_backward=fused)], forward)


def _fused_gan(golden_dir):
    opt = R.gan_opt(pair_bow_dim=211, dropout=0.3)
    z, batch = TG.load(golden_dir)

    def forward(m, s):
        m.set_noise(torch.from_numpy(z[f"eps_e_{s}"]), torch.from_numpy(z[f"eps_c_{s}"]))
        return m(*TG.call(batch, 7 + s))
    return (lambda: TG.build(opt, int(z["meta"][5]), train_dropout=True)[0],
            lambda m, fused: list(m.make_fused_optimizers(fuse_into_backward=fused)), forward)


def _fused_en(golden_dir):
    """The three-space model: the two content-discriminator losses go back as one sum, as in the reference's loop, so the calls line
    up with the six optimisers in the order of tests/test_gpu_en_adv.py::reference_step."""
    opt = OE.OptEn(pair_bow_dim=211, dropout=0.3)
    z, batch = TE.load(golden_dir)

    def forward(m, s):
        eps = TE.eps_of(z, s)
        m.set_noise(eps["con"], eps["e"], eps["c"])
        cd_e, cd_c, ed, ecd, cad, ced, vae = m(*TE.call(batch, 7 + s))
        return (cd_e + cd_c, ed, ecd, cad, ced, vae)

    def optimizers(m, fused):
        o = list(m.make_fused_optimizers(fuse_into_backward=fused))
        return [o[0], o[1], o[3], o[2], o[4], o[5]]
    return lambda: TE.build(opt, int(z["meta"][5]), train_dropout=True)[0], optimizers, forward


def _fused_vi(golden_dir):
    """The vi step (tests/test_gpu_vi.py): torch's Adam on the approximation network, whose _AprxLoss backward sits before every vae
    backward, and FusedAdam on the rest.  (The set-up of that file: dropout 0.)"""
    _, _, z, batch, _, _ = TV._build(golden_dir)

    def build():
        return TV._build(golden_dir)[4]

    def forward(m, s):
        b = {k: v.cuda() for k, v in batch.items()}
        m.set_noise(torch.from_numpy(z[f"eps_e_{s}"]), torch.from_numpy(z[f"eps_c_{s}"]))
        out = m(b["input_ids"], b["attention_masks"], b["token_type_ids"], b["emo_labels"], b["cau_labels"], b["labels"], b["bow_reps"], 5 + s)
        return out[2], out[3]
    return build, (lambda m, fused: [torch.optim.Adam(m.get_params()[0], lr=m.opt.aprx_lr),
                                     M.FusedAdam(m, lr=m.opt.vae_lr, fuse_into_backward=fused)]), forward


FUSED = {"mmd": _fused_mmd, "gan": _fused_gan, "en": _fused_en, "vi": _fused_vi}


@pytest.mark.parametrize("mode", list(FUSED))
def test_fused_adam_stays_out_of_an_accumulating_backward(golden_dir, mode):
    """After tests/test_gpu_model.py::test_adam_fused_into_backward_equals_plain_step: one supported step (each optimiser's zero_grad
    before its loss's backward, then every step(): the fused update does fire), then zero_grad(set_to_none=False) and two micro-batches
    of backward calls onto the standing gradients, then every step() once.  No parameter may move before that step() -- the update
    fused into backward is for a backward that overwrites -- and the weights of the fused and the plain setting agree as that test
    requires of a second step.  The sentence transformer's optimiser has no fused-into-backward form."""
    build, optimizers, forward = FUSED[mode](golden_dir)
    res = {}
    for fused in (False, True):
        model = build()
        model.train()
        opts = optimizers(model, fused)
        adam = opts[-1]
        assert isinstance(adam, M.FusedAdam) and (model._adam_hook is adam) == fused
        losses = forward(model, 0)
        for i, (o, loss) in enumerate(zip(opts, losses)):
            o.zero_grad()
            loss.backward(retain_graph=i != len(losses) - 1)
            if mode == "vi":                     # the reference's vi step updates the approximation network before the vae backward
                o.step()
        if mode != "vi":
            for o in opts:
                o.step()
        model.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        before = model._flat.detach().clone()
        for s in (1, 2):
            losses = forward(model, s)
            for i, loss in enumerate(losses):
                loss.backward(retain_graph=i != len(losses) - 1)
            torch.cuda.synchronize()
            assert torch.equal(model._flat, before), (fused, s, "a parameter moved during an accumulating backward")
        assert adam._done == []
        for o in opts:
            o.step()
        torch.cuda.synchronize()
        assert adam._done == [] and adam.step_count == 2
        res[fused] = ({k: p.detach().clone() for k, p in model.named_parameters()}, before, model)
    moved = 0
    for k, w in res[False][0].items():
        assert relnorm(res[True][0][k], w) <= TM.TOL_FUSED_ADAM_STEP2, k
        o = res[False][2]._offs[k]
        moved += int(not torch.equal(w.reshape(-1), res[False][1][o:o + w.numel()]))
    assert moved >= len(res[False][0]) - 12         # everything optimised did move in the last step (latent heads / a dead pair head stay)
