"""`DrlClassifier`, `MMDStatistic`, `pdist` with the module surface of the reference's
drl_classifier_ec_mmd_final_mul.py (:149-596), executed by the HIP kernels of libcarel_hip.so.

PyTorch's role here is autograd *glue* and memory: one `torch.autograd.Function` spans the whole training
forward (encoder + VAE tail -> scalar loss); its backward enqueues the HIP backward and leaves the
gradients in a flat fp32 buffer that every `Parameter.grad` aliases.  There is no eager/CPU fallback:
calling the model with CPU tensors raises.
"""
import contextlib
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops

H, I_FF, NH = 768, 3072, 12

DEFAULT_OPT = dict(language="zh", max_len=128, e_num_class=6, c_num_class=1, pair_num_class=1, ec_dim=24, bert_dim=768,
                   kl_ann_iterations=20000, epochs=20, batch_size=64, ec_kl_lambda=0.03, label_smoothing=0.1,
                   mmd_loss_weight=30.0, emo_mul_loss_weight=10.0, cau_mul_loss_weight=10.0, pair_mul_loss_weight=30.0,
                   dropout=0.5, epsilon=1e-8, vae_lr=1e-5, aprx_lr=0.003, pair_bow_dim=23771, self_iteration=50, self_epochs=10,
                   self_strategy="random", best_model_path="ECPE_model/best_cause_pair_model", model_id="carel")


def make_opt(**kw):
    """The reference's argparse namespace (:30-61) with its defaults."""
    d = dict(DEFAULT_OPT)
    d.update(kw)
    return SimpleNamespace(**d)


# drl_classifier_ec_gan.py:30-57: the parser defaults of the adversarial (GAN) ablation; the two heads share ec_mul_loss_weight
GAN_OPT = dict(language="zh", max_len=128, ec_num_class=1, e_num_class=1, c_num_class=1, pair_num_class=1, ec_dim=24, con_dim=384,
               pair_bow_dim=23771, bert_dim=768, kl_ann_iterations=20000, epochs=10, batch_size=64, ec_kl_lambda=0.03, con_kl_lambda=0.03,
               label_smoothing=0.1, ecce_adv_loss_weight=1.0, ec_mul_loss_weight=10.0, pair_mul_loss_weight=25.0, dropout=0.5, epsilon=1e-8,
               adv_lr=0.003, vae_lr=1e-5, self_iteration=50, self_epochs=10, self_strategy="random",
               best_model_path="ECPE_model/best_drl_model", model_id="carel-gan", disentangle="gan", emotion_head="bce")
GAN_DISCS = ("ec_disc", "ce_disc")          # get_params() order (:310-317)


def make_gan_opt(**kw):
    """The argparse namespace of drl_classifier_ec_gan.py (:30-57) with its defaults, plus the two switches that select that script's
    model here: disentangle="gan" and the one-logit BCE emotion head (e_num_class / c_num_class mirror its ec_num_class = 1)."""
    d = dict(GAN_OPT)
    d.update(kw)
    return SimpleNamespace(**d)


# drl_classifier_ec_mmd_final_mul_newsplit_emnlp.py:30-75: the parser defaults of the new-split driver (the EMNLP model; the flags stay
# the script's strings).  `confounding` is only printed by the script.
NEWSPLIT_OPT = dict(DEFAULT_OPT, bow_optimize="true", source_domain="home", target_domain="education", bow_file="data/all_data_pair_zh.txt",
                    self_strategy="temporal_order_modification", adapter="false", head_number=4, confounding="false",
                    predicted_emotion="true", round_up="true")


def make_newsplit_opt(**kw):
    """The argparse namespace of drl_classifier_ec_mmd_final_mul_newsplit_emnlp.py (:30-75) with its defaults (plus pair_bow_dim and
    model_id, which the script computes)."""
    d = dict(NEWSPLIT_OPT)
    d.update(kw)
    return SimpleNamespace(**d)


REL_KEY = "encoder.encoder.relative_attention_bias.weight"


def encoder_config(language="zh", **kw):
    """BERT-base geometry of `hfl/chinese-roberta-wwm-ext` (:159) or `roberta-base` (:162); "mpnet": the encoder of
    sentence-transformers/all-mpnet-base-v2 (en_ec_sentence_transformer.py:22; transformers MPNetConfig defaults): RoBERTa-style
    position ids, no token types (type_vocab 1 = an all-zero placeholder row that is never updated) and a learned
    relative-position attention bias [32 buckets, 12 heads] shared by all layers (rel_pos)."""
    if language == "mpnet":
        cfg = dict(vocab_size=30527, max_pos=514, type_vocab=1, ln_eps=1e-5, roberta=1, pad_id=1, rel_pos=True)
    elif language == "en":
        cfg = dict(vocab_size=50265, max_pos=514, type_vocab=1, ln_eps=1e-5, roberta=1, pad_id=1)
    else:
        cfg = dict(vocab_size=21128, max_pos=512, type_vocab=2, ln_eps=1e-12, roberta=0, pad_id=0)
    cfg.setdefault("rel_pos", False)
    cfg.update(layers=12, hidden_dropout=0.1, attn_dropout=0.1)
    cfg.update(kw)
    return SimpleNamespace(**cfg)


# ----------------------------------------------------------------------------------------------
# module tree that reproduces the reference's state_dict key names
# ----------------------------------------------------------------------------------------------
class _Holder(nn.Module):
    """A parameter holder named like the HF / nn.Linear module it stands for (weight [, bias])."""

    def __init__(self, wshape, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(wshape))
        if bias:
            self.bias = nn.Parameter(torch.empty(wshape[0]))


class _Self(nn.Module):
    def __init__(self):
        super().__init__()
        self.query, self.key, self.value = _Holder((H, H)), _Holder((H, H)), _Holder((H, H))


class _SelfOutput(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.dense = _Holder((H, k))
        self.LayerNorm = _Holder((H,))


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.self = _Self()
        self.output = _SelfOutput(H)


class _Intermediate(nn.Module):
    def __init__(self):
        super().__init__()
        self.dense = _Holder((I_FF, H))


class _Layer(nn.Module):
    def __init__(self):
        super().__init__()
        self.attention = _Attention()
        self.intermediate = _Intermediate()
        self.output = _SelfOutput(I_FF)


class _Stack(nn.Module):
    def __init__(self, n, rel_pos=False):
        super().__init__()
        if rel_pos:      # registered BEFORE the layers: in the flat buffer it sits with the embeddings, whose gradients are the last to complete
            self.relative_attention_bias = _Holder((32, NH), bias=False)
        self.layer = nn.ModuleList([_Layer() for _ in range(n)])


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = _Holder((cfg.vocab_size, H), bias=False)
        self.position_embeddings = _Holder((cfg.max_pos, H), bias=False)
        self.token_type_embeddings = _Holder((cfg.type_vocab, H), bias=False)
        self.LayerNorm = _Holder((H,))


class _Pooler(nn.Module):
    def __init__(self):
        super().__init__()
        self.dense = _Holder((H, H))


class _Adapter(nn.Module):
    """Parameter holder with the state_dict keys of the EMNLP scripts' sentence adapters (drl_classifier_ec_mmd_final_mul_emnlp.py):
    nn.MultiheadAttention(768, head_number) for "raw" (:277), and for "sparsemax" / "entmax" its subclasses (:162-256), which add the
    q_proj / k_proj / v_proj linears -- in_proj_* , out_proj and v_proj exist there but only q_proj and k_proj are used."""

    def __init__(self, sparse):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * H, H))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * H))
        self.out_proj = _Holder((H, H))
        if sparse:
            self.q_proj, self.k_proj, self.v_proj = _Holder((H, H)), _Holder((H, H)), _Holder((H, H))


ADAPTERS = ("false", "raw", "sparsemax", "entmax")


def adapter_config(opt):
    """(adapter, head_number) of the EMNLP scripts' --adapter / --head_number (:61-63); "false" (or no attribute): the pooler model."""
    mode = getattr(opt, "adapter", "false")
    if mode is False or mode is None:
        mode = "false"
    heads = getattr(opt, "head_number", 4)
    if mode not in ADAPTERS:
        raise L.CarelError("opt.adapter must be one of %s; got %r" % (", ".join(ADAPTERS), mode))
    if mode == "false":
        return mode, heads
    if int(heads) != heads or heads < 1 or H % int(heads):
        raise L.CarelError("opt.head_number must divide 768 (nn.MultiheadAttention); got %r" % (heads,))
    if mode == "raw" and heads > 12:
        raise L.CarelError("the raw adapter kernels support head_number <= 12; got %d" % heads)
    if getattr(opt, "disentangle", "mmd") != "mmd":
        raise L.CarelError("sentence adapters exist in the MMD scripts only (opt.disentangle must be 'mmd')")
    return mode, int(heads)


def train_adapter_config(opt, adapter):
    """opt.train_adapter (an extension; the reference's get_params() forgets the adapters, :460-473, so they stay at their random
    initialisation there): True / False or the strings "true" / "false", as the scripts pass flags.  Absent: False."""
    v = getattr(opt, "train_adapter", False)
    if isinstance(v, str) and v in ("true", "false"):
        v = v == "true"
    if v is not True and v is not False:
        raise L.CarelError("opt.train_adapter must be True, False, 'true' or 'false'; got %r" % (v,))
    if v and adapter == "false":
        raise L.CarelError("opt.train_adapter needs a sentence adapter (opt.adapter = raw, sparsemax or entmax)")
    return v


# the adapter tensors the forward reads, i.e. the ones opt.train_adapter trains (the sparse subclasses never use in_proj_* / out_proj / v_proj)
ADAPTER_TRAINED = {"raw": ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"),
                   "sparsemax": ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias"),
                   "entmax": ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias")}


class CarelEncoder(nn.Module):
    """Parameter container with the key names of transformers BertModel / RobertaModel."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Stack(cfg.layers, getattr(cfg, "rel_pos", False))
        self.pooler = _Pooler()


def _init_like_reference(model, gen=None):
    """HF init for the encoder (normal(0, 0.02), LayerNorm 1/0, zero biases) and nn.Linear default init
    for the heads; pretrained checkpoints are loaded with load_state_dict (same key names)."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("encoder."):
                if "LayerNorm.weight" in name:
                    p.fill_(1.0)
                elif name.endswith(".bias"):
                    p.zero_()
                else:
                    p.normal_(0.0, 0.02, generator=gen)
            elif "_adapter." in name:       # nn.MultiheadAttention._reset_parameters: xavier in_proj, zero biases; the rest nn.Linear's
                leaf = name.split("_adapter.", 1)[1]
                if leaf == "in_proj_weight":
                    bound = math.sqrt(6.0 / (p.shape[0] + p.shape[1]))
                    p.uniform_(-bound, bound, generator=gen)
                elif leaf in ("in_proj_bias", "out_proj.bias"):
                    p.zero_()
                else:
                    bound = 1.0 / math.sqrt(H)
                    p.uniform_(-bound, bound, generator=gen)
            elif name.endswith(".weight"):
                bound = 1.0 / math.sqrt(p.shape[1])
                p.uniform_(-bound, bound, generator=gen)
            else:
                w = dict(model.named_parameters())[name[:-5] + ".weight"]
                bound = 1.0 / math.sqrt(w.shape[1])
                p.uniform_(-bound, bound, generator=gen)


# ----------------------------------------------------------------------------------------------
# autograd glue
# ----------------------------------------------------------------------------------------------
class _TrainLoss(torch.autograd.Function):
    """Whole-step forward; `anchor` is a dummy requires-grad tensor that makes autograd call backward.
    Gradients are written by the backward kernels straight into model._flat_grad (aliased by every .grad); the classifier / decoder
    gradients, which the forward's loss kernels produce, wait in model._head_img until backward adds them in (_flatten)."""

    @staticmethod
    def forward(ctx, anchor, model, call):
        ctx.model, ctx.call = model, call
        ctx.set_materialize_grads(False)
        model._run_forward(call, training=True)
        # second output: the sampled embeddings [z_e | z_c]; further loss terms built on them (the CLUB bound of the VI
        # ablation, or any torch expression) send their gradient back through `grad_z`
        return call.buf.terms[8].clone(), call.buf.z.clone()

    @staticmethod
    def backward(ctx, grad_out, grad_z):
        if grad_out is None:
            grad_out = ctx.call.buf.terms.new_zeros(())
        ctx.model._run_backward(ctx.call, grad_out, grad_z)
        return None, None, None


class _GanLosses(torch.autograd.Function):
    """Whole-step forward of the GAN ablation returning (ec_disc_loss, ce_disc_loss, vae_and_classifier_loss); each backward call
    receives the upstream gradients of the losses it was started from (None for the others), in the manner of the three-space
    model's _EnLosses: the losses are roots of the graph, every gradient image was produced by the forward kernels."""

    @staticmethod
    def forward(ctx, anchor, model, call):
        ctx.model, ctx.call = model, call
        ctx.set_materialize_grads(False)
        model._run_forward(call, training=True)
        t = call.gan_terms
        return t[0].clone(), t[1].clone(), t[4].clone()

    @staticmethod
    def backward(ctx, g_ec, g_ce, g_vae):
        ctx.model._run_backward_gan(ctx.call, (g_ec, g_ce, g_vae))
        return None, None, None


class _AprxLoss(torch.autograd.Function):
    """`get_ec_aprx_loss` of drl_classifier_ec_vi.py:422-427: loss of the approximation network p(e|c) on the sampled
    embeddings; its backward fills ONLY the eight ec_mu / ec_log_var gradients.  (In the reference the term also sends a
    gradient into the encoder through e_embedding, but `vae_and_cls_opt.zero_grad()` (:771) discards it before use.)"""

    @staticmethod
    def forward(ctx, anchor, model, z):
        ctx.model = model
        loss, ctx.grads = ops.vi_aprx(z, model._aprx_weights())
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        for k, gk in zip(m._aprx_names, ctx.grads):
            view = m._grad_view(k)
            p = m._named[k]
            if p.grad is None:
                view.copy_(gk * g)
            else:
                view.add_(gk * g)
            p.grad = view
        return None, None, None


class _UpperLoss(torch.autograd.Function):
    """`get_ec_upper_loss` (:429-440): CLUB upper bound of I(e; c) with the negatives e[randperm]."""

    @staticmethod
    def forward(ctx, e, c, model, perm):
        D = e.shape[1]
        z = torch.cat((e, c), dim=1).float().contiguous()
        loss, dz = ops.vi_upper(z, model._aprx_weights(), perm)
        ctx.save_for_backward(dz)
        ctx.D = D
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dz, = ctx.saved_tensors
        dz = dz * g
        return dz[:, :ctx.D], dz[:, ctx.D:], None, None


class _MMDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s1, s2, alphas, ret_matrix):
        s1c, s2c = s1.contiguous().float(), s2.contiguous().float()
        out, kern = ops.rbf_mmd(s1c, s2c, alphas, ret_matrix=ret_matrix)
        ctx.save_for_backward(s1c, s2c)
        ctx.alphas = alphas
        if ret_matrix:
            ctx.mark_non_differentiable(kern)
            return out.reshape(()), kern
        return out.reshape(())

    @staticmethod
    def backward(ctx, g, *unused):
        s1, s2 = ctx.saved_tensors
        g1, g2 = ops.rbf_mmd_backward(s1, s2, ctx.alphas, g.reshape(1).float())
        return g1, g2, None, None


class _HSICFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, s_x, s_y):
        xc, yc = x.contiguous().float(), y.contiguous().float()
        ctx.save_for_backward(xc, yc)
        ctx.s = (s_x, s_y)
        return ops.hsic(xc, yc, s_x, s_y).reshape(())

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx, gy = ops.hsic_backward(x, y, g, *ctx.s)
        return gx, gy, None, None


def HSIC(x, y, s_x=1, s_y=1):
    """Drop-in for `HSIC` of the ablation script drl_classifier_ec_hsic.py:540-547 (HIP kernel, differentiable)."""
    return _HSICFn.apply(x, y, float(s_x), float(s_y))


class MMDStatistic:
    """Drop-in for the reference's `MMDStatistic` (:537-577); `__call__` runs the HIP RBF-MMD kernel."""

    def __init__(self, n_1, n_2):
        self.n_1, self.n_2 = n_1, n_2
        self.a00 = 1. / (n_1 * (n_1 - 1))
        self.a11 = 1. / (n_2 * (n_2 - 1))
        self.a01 = - 1. / (n_1 * n_2)

    def __call__(self, sample_1, sample_2, alphas, ret_matrix=False):
        if sample_1.shape[0] != self.n_1 or sample_2.shape[0] != self.n_2:
            raise ValueError("sample sizes differ from the constructor's n_1/n_2")
        ops._chk_cuda(sample_1, sample_2)
        return _MMDFn.apply(sample_1, sample_2, [float(a) for a in alphas], bool(ret_matrix))

    def pval(self, distances, n_permutations=1000, *, labels=None, generator=None, return_stats=False):
        """The reference's `pval` (:571-577) on the matrix that `__call__(..., ret_matrix=True)` or `ops.rbf_gram` returns: the
        permutation p-value of the statistic, a Python float (`permutation_test_mat`; the reference calls a stub there)."""
        return permutation_test_mat(distances, self.n_1, self.n_2, n_permutations, a00=self.a00, a11=self.a11, a01=self.a01,
                                    labels=labels, generator=generator, return_stats=return_stats)


def random_labellings(n_1, n_2, n_permutations, device, generator=None):
    """uint8 [n_permutations + 1, n_1 + n_2] on `device`: the observed labelling [0] * n_1 + [1] * n_2 first, then uniformly random
    labellings with n_2 ones each -- the first n_2 places of a stable argsort of uniform draws, so a seeded generator repeats them
    (the draws are made on the generator's own device)."""
    n, P = n_1 + n_2, int(n_permutations)
    labels = torch.zeros((P + 1, n), dtype=torch.uint8, device=device)
    labels[0, n_1:] = 1
    u = torch.rand((P, n), generator=generator, device=device if generator is None else generator.device)
    labels[1:].scatter_(1, torch.argsort(u, dim=1, stable=True)[:, :n_2].to(device), 1)
    return labels


def permutation_test_mat(matrix, n_1, n_2, n_permutations, a00=1, a01=0, a11=1, *, labels=None, generator=None, return_stats=False):
    """The reference's stub (:599-600) filled in; THE DEFINITION IS THIS PROJECT'S OWN (include/carel_hip.h, carel_mmd_perm_test).
    stat(g) = sum over i != j of c(g_i, g_j) matrix[i, j] with c(0,0) = a00, c(1,1) = a11, c(0,1) = c(1,0) = a01; the p-value is the
    share of the n_permutations relabellings whose statistic is >= the observed one's (labelling [0] * n_1 + [1] * n_2, not itself
    among them).  matrix: [n, n] CUDA tensor, CPU tensor or ndarray (it goes to the device as float32).  labels: uint8
    [n_permutations, n] relabellings with n_2 ones each (default: `random_labellings` from `generator`).  Returns a Python float, with
    return_stats (pval, stats float64 [n_permutations + 1] on the device, count)."""
    if not torch.cuda.is_available():
        raise L.CarelError("permutation_test_mat runs on the GPU (carel_mmd_perm_test); there is no CPU fallback.")
    m = torch.as_tensor(matrix).detach()
    dev = m.device if m.is_cuda else torch.device("cuda", torch.cuda.current_device())
    m = m.to(dev, torch.float32)
    n_1, n_2, P = int(n_1), int(n_2), int(n_permutations)
    n = n_1 + n_2
    if n_1 < 2 or n_2 < 2 or n > L.PERM_MAX_N or not 1 <= P <= L.PERM_MAX_PERMUTATIONS:
        raise L.CarelError("permutation_test_mat: n_1, n_2 >= 2, n_1 + n_2 <= %d and 1 <= n_permutations <= %d are required"
                           % (L.PERM_MAX_N, L.PERM_MAX_PERMUTATIONS))
    if m.dim() != 2 or tuple(m.shape) != (n, n):
        raise L.CarelError("permutation_test_mat: the matrix must be [n_1 + n_2, n_1 + n_2]")
    if m.stride(1) != 1:
        m = m.contiguous()
    with torch.cuda.device(dev):
        if labels is None:
            full = random_labellings(n_1, n_2, P, dev, generator)
        else:
            lab = torch.as_tensor(labels)
            if lab.dtype != torch.uint8 or tuple(lab.shape) != (P, n):
                raise L.CarelError("permutation_test_mat: labels must be uint8 [n_permutations, n_1 + n_2]")
            lab = lab.to(dev)
            if bool((lab > 1).any()) or bool((lab.sum(dim=1, dtype=torch.int64) != n_2).any()):
                raise L.CarelError("permutation_test_mat: every row of labels must hold exactly n_2 ones and zeros otherwise")
            full = torch.cat((random_labellings(n_1, n_2, 0, dev)[:1], lab), 0)
        stats, count = ops.mmd_perm_test(m, full, n_1, n_2, a00, a01, a11)
        c = int(count.item())
    pval = c / P
    return (pval, stats, c) if return_stats else pval


MEDIAN = "median"


def _is_median(who, name, value):
    """True for the string "median"; any other string is refused by name (on every machine, before anything else is looked at)"""
    if not isinstance(value, str):
        return False
    if value != MEDIAN:
        raise L.CarelError('%s: %s = %r is not a width; the only accepted word is "%s" (the median heuristic), otherwise give numbers'
                           % (who, name, value, MEDIAN))
    return True


def pdist_quantile(x, q=0.5):
    """The q-quantile of the squared pairwise distances { D_ij : i < j } of the rows of x [m, d] (2 <= m <= 8192, d <= 64) by numpy's
    default ("linear") rule, a Python float: the two neighbouring order statistics are selected exactly on the device
    (carel_pdist_select -- the distances `hsic_gram` exponentiates, bit for bit; the matrix is never stored) and interpolated in
    double on the host.  One read-back.  THE DEFINITION IS THIS PROJECT'S OWN (the reference has no such function)."""
    if not torch.cuda.is_available():
        raise L.CarelError("pdist_quantile runs on the GPU (carel_pdist_select); there is no CPU fallback.")
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise L.CarelError("pdist_quantile: q must lie in [0, 1] (got %r)" % q)
    xs = torch.as_tensor(x).detach()
    dev = xs.device if xs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    xs = xs.to(dev, torch.float32)
    if xs.dim() != 2 or xs.shape[0] < 2:
        raise L.CarelError("pdist_quantile: a sample [m, d] of at least 2 rows is required")
    if xs.stride(1) != 1:
        xs = xs.contiguous()
    n_pairs = xs.shape[0] * (xs.shape[0] - 1) // 2
    pos = (n_pairs - 1) * q
    lo = min(int(math.floor(pos)), n_pairs - 1)
    hi = min(lo + 1, n_pairs - 1)
    with torch.cuda.device(dev):
        values, _ = ops.pdist_select(xs, [lo, hi])
        v_lo, v_hi = (float(v) for v in values.double().cpu())
    return v_lo + (v_hi - v_lo) * (pos - lo)


def median_heuristic(x):
    """The median-heuristic kernel width of a sample (Gretton et al.): the median squared pairwise distance, `pdist_quantile(x, 0.5)`."""
    return pdist_quantile(x, 0.5)


def _median_width(who, name, sample):
    med = median_heuristic(sample)
    if not med > 0.0:
        raise L.CarelError("%s: the median squared distance behind %s is %r, not > 0 (more than half of the pairs of rows coincide): "
                           "there is no median-heuristic width; give a number" % (who, name, med))
    return med


def median_alphas(sample_1, sample_2, scales=(1.0,)):
    """[1 / (scale * median)] for every scale: the `alphas` of the median heuristic for `mmd_two_sample_test` and
    `MMDStatistic.__call__`, median = `median_heuristic` of the pooled sample [sample_1; sample_2] (the squared distances of
    `hsic_gram`: no eps, no abs -- 1e-5 away from the MMD kernel's own argument, immaterial to a heuristic)."""
    if not torch.cuda.is_available():
        raise L.CarelError("median_alphas runs on the GPU (carel_pdist_select); there is no CPU fallback.")
    s1, s2 = torch.as_tensor(sample_1).detach(), torch.as_tensor(sample_2).detach()
    dev = s1.device if s1.is_cuda else (s2.device if s2.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    if s1.dim() != 2 or s2.dim() != 2 or s1.shape[1] != s2.shape[1]:
        raise L.CarelError("median_alphas: two samples [n_1, d], [n_2, d] are required")
    med = _median_width("median_alphas", "the pooled sample", torch.cat((s1.to(dev, torch.float32), s2.to(dev, torch.float32)), 0))
    return [1.0 / (float(s) * med) for s in scales]


def mmd_two_sample_test(sample_1, sample_2, alphas, n_permutations=1000, eps=1e-5, labels=None, generator=None, return_stats=False,
                        return_widths=False):
    """The two-sample test from the samples: the tiled Gram matrix (carel_rbf_gram, n_1 + n_2 <= 8192), then `permutation_test_mat`
    with MMDStatistic's coefficients.  Returns (mmd, pval) as Python floats -- mmd is the observed statistic, what
    MMDStatistic.__call__ computes -- and with return_stats (mmd, pval, stats, count).  alphas = "median": `median_alphas` of the two
    samples, [1 / median squared distance of the pooled sample].  return_widths appends {"alphas": the list used}."""
    median = _is_median("mmd_two_sample_test", "alphas", alphas)
    if not torch.cuda.is_available():
        raise L.CarelError("mmd_two_sample_test runs on the GPU (carel_rbf_gram, carel_mmd_perm_test); there is no CPU fallback.")
    s1, s2 = torch.as_tensor(sample_1).detach(), torch.as_tensor(sample_2).detach()
    dev = s1.device if s1.is_cuda else (s2.device if s2.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    s1, s2 = s1.to(dev, torch.float32), s2.to(dev, torch.float32)
    if s1.dim() != 2 or s2.dim() != 2:
        raise L.CarelError("mmd_two_sample_test: two [n, d] samples are required")
    s1, s2 = (s if s.stride(1) == 1 else s.contiguous() for s in (s1, s2))
    if s1.shape[0] < 2 or s2.shape[0] < 2:
        raise L.CarelError("mmd_two_sample_test: both samples need at least 2 rows")
    stat = MMDStatistic(s1.shape[0], s2.shape[0])
    alphas = median_alphas(s1, s2) if median else [float(a) for a in alphas]
    with torch.cuda.device(dev):
        kern = ops.rbf_gram(s1, s2, alphas, eps)
    pval, stats, count = stat.pval(kern, n_permutations, labels=labels, generator=generator, return_stats=True)
    mmd = float(stats[0])
    out = (mmd, pval, stats, count) if return_stats else (mmd, pval)
    return out + (dict(alphas=alphas),) if return_widths else out


def random_permutations(m, n_permutations, device, generator=None):
    """int32 [n_permutations + 1, m] on `device`: the identity first (the observed pairing), then uniformly random permutations of
    0..m-1 -- the stable argsort of uniform draws, so a seeded generator repeats them (the draws are made on the generator's own
    device)."""
    m, P = int(m), int(n_permutations)
    perms = torch.empty((P + 1, m), dtype=torch.int32, device=device)
    perms[0] = torch.arange(m, dtype=torch.int32, device=device)
    u = torch.rand((P, m), generator=generator, device=device if generator is None else generator.device)
    perms[1:] = torch.argsort(u, dim=1, stable=True).to(device, torch.int32)
    return perms


def _checked_permutations(who, permutations, P, m, dev):
    """int32 [P, m] on `dev`, or CarelError: the shape and the dtype on the host, then -- one reduction and one read-back -- every sorted
    row against arange(m) on the device"""
    pm = torch.as_tensor(permutations)
    if pm.dtype not in (torch.int32, torch.int64) or tuple(pm.shape) != (P, m):
        raise L.CarelError("%s: permutations must be int32 or int64 [n_permutations, m]" % who)
    pm = pm.to(dev)
    if not bool((torch.sort(pm, dim=1).values == torch.arange(m, device=dev, dtype=pm.dtype)).all()):
        raise L.CarelError("%s: every row of permutations must be a permutation of 0..m-1" % who)
    return pm.to(torch.int32)


def hsic_permutation_test(K, L_, n_permutations=1000, *, permutations=None, generator=None, return_stats=False, _checked=False):
    """The permutation independence test of Gretton et al. (2007) on two kernel matrices; THE DEFINITION IS THIS PROJECT'S OWN
    (include/carel_hip.h, carel_hsic_perm_test; the reference has no such function, the statistic is its HSIC).  With Kc = H K H,
    stat(pi) = sum_ij Kc[i, j] L[pi_i, pi_j] / (m-1)^2; the p-value is the share of the n_permutations re-pairings whose statistic is
    >= the observed one's (pi = identity, not itself among them).  K, L: [m, m] CUDA tensors, CPU tensors or ndarrays (they go to the
    device as float32), 2 <= m <= 8192.  permutations: int32 / int64 [n_permutations, m] re-pairings (default: `random_permutations`
    from `generator`); they are validated on the device -- every sorted row must equal arange(m) -- which costs one reduction and one
    read-back before the test is launched.  Returns a Python float, with return_stats (pval, stats float64 [n_permutations + 1] on
    the device, count)."""
    if not torch.cuda.is_available():
        raise L.CarelError("hsic_permutation_test runs on the GPU (carel_hsic_perm_test); there is no CPU fallback.")
    k, l = torch.as_tensor(K).detach(), torch.as_tensor(L_).detach()
    dev = k.device if k.is_cuda else (l.device if l.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    k, l = k.to(dev, torch.float32), l.to(dev, torch.float32)
    P = int(n_permutations)
    if k.dim() != 2 or k.shape[0] != k.shape[1] or tuple(l.shape) != tuple(k.shape):
        raise L.CarelError("hsic_permutation_test: K and L must both be [m, m]")
    m = k.shape[0]
    if not 2 <= m <= L.HSIC_PERM_MAX_M or not 1 <= P <= L.PERM_MAX_PERMUTATIONS:
        raise L.CarelError("hsic_permutation_test: 2 <= m <= %d and 1 <= n_permutations <= %d are required"
                           % (L.HSIC_PERM_MAX_M, L.PERM_MAX_PERMUTATIONS))
    k, l = (t if t.stride(1) == 1 else t.contiguous() for t in (k, l))
    with torch.cuda.device(dev):
        if permutations is None:
            full = random_permutations(m, P, dev, generator)
        else:
            pm = permutations if _checked else _checked_permutations("hsic_permutation_test", permutations, P, m, dev)
            full = torch.cat((torch.arange(m, device=dev, dtype=torch.int32)[None], pm), 0)
        stats, count = ops.hsic_perm_test(k, l, full)
        c = int(count.item())
    pval = c / P
    return (pval, stats, c) if return_stats else pval


def hsic_independence_test(x, y, s_x=1.0, s_y=1.0, n_permutations=1000, *, permutations=None, generator=None, return_stats=False,
                           return_widths=False):
    """The independence test from the paired samples x [m, d_x], y [m, d_y] (the widths may differ): the tiled Gram matrices
    K = exp(-D(x) / s_x), L = exp(-D(y) / s_y) (carel_hsic_gram, 2 <= m <= 8192), then `hsic_permutation_test`.  Returns (hsic, pval)
    as Python floats -- hsic is the observed statistic, what `HSIC(x, y, s_x, s_y)` computes (differentiably, up to the same 8192
    rows; here from the stored matrices in double) -- and with return_stats (hsic, pval, stats, count).  s_x / s_y = "median": the
    `median_heuristic` of that sample (a median that is not > 0 is refused).  return_widths appends {"s_x": ..., "s_y": ...}, the
    widths used."""
    med_x, med_y = _is_median("hsic_independence_test", "s_x", s_x), _is_median("hsic_independence_test", "s_y", s_y)
    if not torch.cuda.is_available():
        raise L.CarelError("hsic_independence_test runs on the GPU (carel_hsic_gram, carel_hsic_perm_test); there is no CPU fallback.")
    xs, ys = torch.as_tensor(x).detach(), torch.as_tensor(y).detach()
    dev = xs.device if xs.is_cuda else (ys.device if ys.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    xs, ys = xs.to(dev, torch.float32), ys.to(dev, torch.float32)
    if xs.dim() != 2 or ys.dim() != 2 or xs.shape[0] != ys.shape[0]:
        raise L.CarelError("hsic_independence_test: two samples [m, d_x], [m, d_y] of the same number of rows are required")
    xs, ys = (s if s.stride(1) == 1 else s.contiguous() for s in (xs, ys))
    with torch.cuda.device(dev):
        if permutations is not None:         # refused before the Gram launches, not after them
            permutations = _checked_permutations("hsic_independence_test", permutations, int(n_permutations), xs.shape[0], dev)
        if med_x:
            s_x = _median_width("hsic_independence_test", "s_x", xs)
        if med_y:
            s_y = _median_width("hsic_independence_test", "s_y", ys)
        kx, ky = ops.hsic_gram(xs, s_x), ops.hsic_gram(ys, s_y)
    pval, stats, count = hsic_permutation_test(kx, ky, n_permutations, permutations=permutations, generator=generator, return_stats=True,
                                               _checked=permutations is not None)
    hsic = float(stats[0])
    out = (hsic, pval, stats, count) if return_stats else (hsic, pval)
    return out + (dict(s_x=float(s_x), s_y=float(s_y)),) if return_widths else out


class _PdistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s1, s2, eps):
        s1c, s2c = s1.contiguous().float(), s2.contiguous().float()
        ctx.save_for_backward(s1c, s2c)
        ctx.eps = eps
        return ops.pdist(s1c, s2c, eps)

    @staticmethod
    def backward(ctx, g):
        s1, s2 = ctx.saved_tensors
        g1, g2 = ops.pdist_backward(s1, s2, g, ctx.eps)
        return g1, g2, None


def pdist(sample_1, sample_2, norm=2, eps=1e-5):
    """Reference `pdist` (:580-596), L2 only (the only live branch): sqrt(eps + |d2|) from the squared distance itself
    (HIP kernel `carel_pdist_fwd`, differentiable) -- no exp / log round trip, so samples that are far apart (d2 > 100,
    where exp(-d2) underflows in fp32) and samples that nearly coincide both come out to fp32 rounding."""
    if float(norm) != 2.:
        raise NotImplementedError("only norm=2 is on the hot path (:583)")
    ops._chk_cuda(sample_1, sample_2)
    return _PdistFn.apply(sample_1, sample_2, float(eps))


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------
class _Call:
    """Everything one forward/backward pair shares."""
    pass



def rel_span(S):
    """Entries of the MPNet bias-by-distance row the attention kernels read at length S: 256 (S <= 128), 1024 (S > 128)."""
    return 256 if S <= 128 else 1024


def mpnet_bucket_by_distance(span):
    """int32 [span]: entry i = transformers MPNetEncoder.relative_position_bucket of the distance key - query = i - (span/2 - 1)
    (num_buckets 32, max_distance 128; the same float32 log and truncation); the last entry is unused."""
    rel = torch.arange(-(span // 2 - 1), span // 2 + 1, dtype=torch.long)
    n = -rel
    ret = (n < 0).to(torch.long) * 16
    n = torch.abs(n)
    large = 8 + (torch.log(n.float() / 8) / math.log(128 / 8) * 8).to(torch.long)
    ret = ret + torch.where(n < 8, n, torch.min(large, torch.full_like(large, 15)))
    return ret.to(torch.int32)

class DrlClassifier(nn.Module):
    """Reference `DrlClassifier` (:149-534).  Same constructor argument, attribute names, `forward`,
    `get_pair_preds`, `get_params`, state_dict keys."""

    TERM_NAMES = ("partial", "mmd", "emo", "cau", "pair", "kl_e", "kl_c", "rec", "loss")

    def __init__(self, opt, encoder_cfg=None, seed=None):
        super().__init__()
        self.opt = opt
        self.cfg = encoder_cfg if encoder_cfg is not None else encoder_config(getattr(opt, "language", "zh"))
        if opt.bert_dim != H:
            raise L.CarelError("bert_dim must be 768 (BERT-base kernels)")
        self.adapter, self.head_number = adapter_config(opt)
        self.train_adapter = train_adapter_config(opt, self.adapter)
        self.encoder = CarelEncoder(self.cfg)
        self._aprx_names = []
        self._adapter_names = []
        self._adapter_train_names = []      # opt.train_adapter: the subset of _adapter_names that gets a gradient and sits in the optimised prefix
        self._disc_names = []               # the two adversaries of opt.disentangle == "gan" (fp32 only, own optimisers)
        self._gan = getattr(opt, "disentangle", "mmd") == "gan"
        self._has_pair_skip = True          # the pair head is frozen for a step whose pair loss was replaced by 0 (ref :510-511)
        self.strict_pair_skip = False       # True: also leave its .grad None on such a step (for stock torch optimisers; one host read per step)
        self._build_heads(opt)
        gen = None
        if seed is not None:
            gen = torch.Generator().manual_seed(seed)
        _init_like_reference(self, gen)
        if self.adapter != "false":
            # fixed queries (:275, :284): not parameters, not in the state_dict; drawn from the model's generator, assignable
            self.register_buffer("emotion_q", torch.randn(1, 1, H, generator=gen), persistent=False)
            self.register_buffer("cause_q", torch.randn(1, 1, H, generator=gen), persistent=False)
        self.dropout_base_seed = 0x5EED
        self.varlen = True                   # skip padded positions (results identical; see _pack_info)
        self.cls_only_last = True            # last layer's row-wise half on the [CLS] rows only (results identical)
        self.overlap_wgrad = True            # weight-gradient GEMMs on a second stream beside the dgrad chain (results identical)
        self.forward_chains = False          # dense batches: the two halves of the batch as two forward chains on two streams (results
                                             # identical; opt-in: ~1 % slower than one chain since the round-2 GEMMs fill the chip)
        self.debug_fp32 = False              # forward-only measurement mode: the encoder in fp32 (carel_encoder_forward_f32), dropout off;
                                             # forward_terms() / forward() under torch.no_grad() only -- separates bf16 rounding from kernel error
        self._fwd_count = 0
        self._noise = None
        self._ws = {}                        # small per-shape buffers (tail, [CLS] index arrays)
        self._enc_ws = {}                    # encoder activation / scratch workspaces, LRU-bounded (see _workspace)
        self._dp = None                     # set by carel_vae_amd.dp.DataParallel
        self._adam_hook = None              # set by FusedAdam(fuse_into_backward=True)
        self._flat = None
        self._flatten()

    def _build_heads(self, opt):
        if self.adapter != "false":         # registered where the reference builds them (:273-291): before the latent heads
            self.emotion_adapter = _Adapter(self.adapter != "raw")
            self.cause_adapter = _Adapter(self.adapter != "raw")
            self._adapter_names = ["%s_adapter.%s" % (side, n) for side in ("emotion", "cause")
                                   for n, _ in getattr(self, side + "_adapter").named_parameters()]
            if self.train_adapter:
                self._adapter_train_names = ["%s_adapter.%s" % (side, n) for side in ("emotion", "cause") for n in ADAPTER_TRAINED[self.adapter]]
        self.emotion_mu = _Holder((opt.ec_dim, H))
        self.emotion_log_var = _Holder((opt.ec_dim, H))
        self.cause_mu = _Holder((opt.ec_dim, H))
        self.cause_log_var = _Holder((opt.ec_dim, H))
        if self._gan:                       # registered where drl_classifier_ec_gan.py builds them (:168-169): state_dict keys in its order
            counts = [getattr(opt, n, 1) for n in ("e_num_class", "c_num_class", "pair_num_class", "ec_num_class")]
            if getattr(opt, "emotion_head", "ce") != "bce" or any(c != 1 for c in counts):
                raise L.CarelError("opt.disentangle == 'gan' is the one-logit model of drl_classifier_ec_gan.py: it needs "
                                   "opt.emotion_head == 'bce' and e_num_class = c_num_class = pair_num_class = ec_num_class = 1; got "
                                   "emotion_head %r, class counts %r" % (getattr(opt, "emotion_head", "ce"), counts))
            self.ec_disc, self.ce_disc = _Holder((1, opt.ec_dim)), _Holder((1, opt.ec_dim))
            self._disc_names = [g + t for g in GAN_DISCS for t in (".weight", ".bias")]
        self.emotion_classifier = _Holder((opt.e_num_class, opt.ec_dim))
        self.cause_classifier = _Holder((opt.c_num_class, opt.ec_dim))
        self.pair_classifier = _Holder((opt.pair_num_class, opt.ec_dim * 2))
        self.decoder = _Holder((opt.pair_bow_dim, opt.ec_dim * 2))
        self.dropout = nn.Dropout(opt.dropout)       # probability holder; the mask is drawn in-kernel
        if getattr(opt, "disentangle", "mmd") == "vi":      # approximation network p(e|c), drl_classifier_ec_vi.py:156-163
            D = opt.ec_dim
            self.ec_mu = nn.Sequential(nn.Linear(D, D), nn.ReLU(), nn.Linear(D, D))
            self.ec_log_var = nn.Sequential(nn.Linear(D, D), nn.ReLU(), nn.Linear(D, D), nn.Tanh())
            self._aprx_names = [f"{n}.{i}.{t}" for n in ("ec_mu", "ec_log_var") for i in (0, 2) for t in ("weight", "bias")]

    # ------------------------------------------------------------------ flat parameter storage
    def _param_order(self):
        """Flat layout: optimised tensors first (so fused Adam is one contiguous range), the four latent
        heads (never optimised, ref :292-295) last; q/k/v weights and biases adjacent (fused QKV GEMM)."""
        order, _, named = self._param_order_encoder()
        order += ["encoder.pooler.dense.weight", "encoder.pooler.dense.bias", "decoder.weight", "decoder.bias",
                  "emotion_classifier.weight", "emotion_classifier.bias", "cause_classifier.weight", "cause_classifier.bias"]
        self._pair_range_names = ["pair_classifier.weight", "pair_classifier.bias"]
        order += self._pair_range_names
        order += self._adapter_train_names   # opt.train_adapter: inside the one range FusedAdam(model) covers
        n_opt_names = len(order)
        order += self._disc_names            # gan: [vae group | ec_disc | ce_disc | latent heads], each optimiser group one contiguous range
        order += ["emotion_mu.weight", "emotion_mu.bias", "emotion_log_var.weight", "emotion_log_var.bias",
                  "cause_mu.weight", "cause_mu.bias", "cause_log_var.weight", "cause_log_var.bias"]
        # frozen like the latent heads (absent from get_params() in the reference, :460); with opt.train_adapter: the ones the forward never reads
        order += [k for k in self._adapter_names if k not in self._adapter_train_names]
        order += self._aprx_names            # own optimiser (ref ec_vi :873), fp32 only
        assert set(order) == set(named), "parameter inventory mismatch"
        return order, n_opt_names, named

    def _param_order_encoder(self):
        """Embeddings and encoder layers (q/k/v weights and biases adjacent: fused QKV GEMM); (order, None, named)."""
        named = dict(self.named_parameters())
        order = []
        e = "encoder.embeddings."
        order += [e + "word_embeddings.weight", e + "position_embeddings.weight", e + "token_type_embeddings.weight",
                  e + "LayerNorm.weight", e + "LayerNorm.bias"]
        if getattr(self.cfg, "rel_pos", False):
            order.append(REL_KEY)            # with the embeddings: complete only after the LAST layer's backward, like them
        for l in range(self.cfg.layers):
            p = f"encoder.encoder.layer.{l}."
            order += [p + "attention.self.query.weight", p + "attention.self.key.weight", p + "attention.self.value.weight",
                      p + "attention.self.query.bias", p + "attention.self.key.bias", p + "attention.self.value.bias",
                      p + "attention.output.dense.weight", p + "attention.output.dense.bias",
                      p + "attention.output.LayerNorm.weight", p + "attention.output.LayerNorm.bias",
                      p + "intermediate.dense.weight", p + "intermediate.dense.bias",
                      p + "output.dense.weight", p + "output.dense.bias", p + "output.LayerNorm.weight", p + "output.LayerNorm.bias"]
        return order, None, named

    def _flatten(self):
        order, n_opt_names, named = self._param_order()
        dev = next(iter(named.values())).device
        offs, o = {}, 0
        for i, k in enumerate(order):
            if i == n_opt_names:
                self._n_opt = o
            offs[k] = o
            o += (named[k].numel() + 63) & ~63        # 256-byte aligned segments
        flat = torch.empty(o, device=dev, dtype=torch.float32)
        flat.zero_()
        with torch.no_grad():
            for k in order:
                p = named[k]
                seg = flat[offs[k]:offs[k] + p.numel()].view(p.shape)
                seg.copy_(p.data.to(torch.float32))
                p.data = seg
        self._flat, self._offs, self._order = flat, offs, order
        self._named = named
        self._flat_grad = torch.zeros_like(flat) if dev.type == "cuda" else None
        self._shadow = torch.empty(o, device=dev, dtype=torch.bfloat16) if dev.type == "cuda" else None
        self._shadow_versions = None
        self._grad_views = None
        self._layer_structs = None
        self._ws = {}
        self._enc_ws = {}
        self._pair_lo = offs[self._pair_range_names[0]]
        self._pair_hi = offs[self._pair_range_names[1]] + named[self._pair_range_names[1]].numel()
        # the classifier / decoder gradients come out of the FORWARD's loss kernels (for grad_output = 1).  They are written to an image of
        # their range beside the gradient buffer, so that a forward leaves every .grad alone; the backward adds grad_output x the image
        # into the range (or overwrites it), like the adversaries' images of the gan model
        self._head_range = self._head_grad_range()
        self._head_img = torch.zeros(self._head_range[1] - self._head_range[0], device=dev) if dev.type == "cuda" else None
        if getattr(self, "_gan", False):
            end = lambda k: offs[k] + ((named[k].numel() + 63) & ~63)        # noqa: E731
            self._group_ranges = {"vae": (0, self._n_opt)}
            for g in GAN_DISCS:
                self._group_ranges[g] = (offs[g + ".weight"], end(g + ".bias"))
            self._disc_lo, self._disc_hi = self._group_ranges[GAN_DISCS[0]][0], self._group_ranges[GAN_DISCS[-1]][1]
            # gradient images of the discriminator range for unit upstream gradients: [0] own loss, [1] entropy term (carel_gan_disc)
            self._disc_img = [torch.zeros(self._disc_hi - self._disc_lo, device=dev) for _ in range(2)] if dev.type == "cuda" else None

    def _head_grad_range(self):
        """[lo, hi) of the flat buffer that holds the gradients the loss kernels produce: decoder .. pair classifier."""
        return self._offs["decoder.weight"], self._pair_hi

    def _head_img_view(self, k):
        p = self._named[k]
        o = self._offs[k] - self._head_range[0]
        return self._head_img[o:o + p.numel()].view(p.shape)

    def _g_head(self, key):
        return self._head_img.data_ptr() + (self._offs[key] - self._head_range[0]) * 4

    def _apply(self, fn, *a, **kw):
        r = super()._apply(fn, *a, **kw)
        self._flatten()
        return r

    def load_state_dict(self, state_dict, strict=True, **kw):
        # buffers such as HF's `encoder.embeddings.position_ids` are not parameters here
        sd = {k: v for k, v in state_dict.items() if not k.endswith(("position_ids", "token_type_ids"))}
        with torch.no_grad():
            r = super().load_state_dict(sd, strict=strict, **kw)
        self._shadow_versions = None
        return r

    def get_params(self):
        """Reference order (:292-295): encoder, decoder, emotion / cause / pair classifiers.  The four latent
        heads are deliberately absent (they are never updated in the reference).
        With opt.disentangle == "vi": the pair (ec_aprx_params, other_params) of drl_classifier_ec_vi.py:291-302."""
        other = (list(self.encoder.parameters()) + list(self.decoder.parameters()) +
                 list(self.emotion_classifier.parameters()) + list(self.cause_classifier.parameters()) +
                 list(self.pair_classifier.parameters()))
        if self._aprx_names:
            return list(self.ec_mu.parameters()) + list(self.ec_log_var.parameters()), other
        if self._gan:            # (ec_disc_params, ce_disc_params, other_params), drl_classifier_ec_gan.py:302-317
            return list(self.ec_disc.parameters()), list(self.ce_disc.parameters()), other
        return other + [self._named[k] for k in self._adapter_train_names]     # opt.train_adapter (extension): the reference's list, then the adapters

    def make_fused_optimizers(self, adv_lr=None, vae_lr=None, fuse_into_backward=False):
        """opt.disentangle == "gan": the three optimisers of drl_classifier_ec_gan.py's script body (:903-908) as HIP kernels over the flat
        buffer, in get_params() order: RMSprop(adv_lr) for ec_disc and for ce_disc, Adam(vae_lr) for the rest."""
        if not self._gan:
            raise L.CarelError("make_fused_optimizers() belongs to opt.disentangle == 'gan' (use FusedAdam(model) otherwise)")
        adv_lr = self.opt.adv_lr if adv_lr is None else adv_lr
        vae_lr = self.opt.vae_lr if vae_lr is None else vae_lr
        groups = self.get_params()
        opts = [FusedRMSprop(self, lr=adv_lr, param_range=self._group_ranges[g], params=groups[i]) for i, g in enumerate(GAN_DISCS)]
        opts.append(FusedAdam(self, lr=vae_lr, param_range=self._group_ranges["vae"], params=groups[2], fuse_into_backward=fuse_into_backward))
        return tuple(opts)

    def _aprx_weights(self):
        if not self._aprx_names:
            raise L.CarelError("the approximation network exists only with opt.disentangle == 'vi'")
        return [self._named[k].data for k in self._aprx_names]

    def get_ec_aprx_loss(self, e_embedding, c_embedding):
        """drl_classifier_ec_vi.py:422-427 (the cause embedding is detached there; only the network gets a gradient)."""
        z = torch.cat((e_embedding.detach(), c_embedding.detach()), dim=1).float().contiguous()
        if not torch.is_grad_enabled():
            return ops.vi_aprx(z, self._aprx_weights())[0].reshape(())
        return _AprxLoss.apply(self._flat.new_zeros((), requires_grad=True), self, z)

    def get_ec_upper_loss(self, e_embedding, c_embedding, random_index=None):
        """drl_classifier_ec_vi.py:429-440.  random_index (extension): the permutation to use instead of a fresh
        torch.randperm(batch) (drawn on the host generator like the reference)."""
        n = e_embedding.shape[0]
        perm = torch.randperm(n) if random_index is None else random_index
        perm = perm.to(e_embedding.device, torch.int32).contiguous()
        return _UpperLoss.apply(e_embedding, c_embedding, self, perm)

    # ------------------------------------------------------------------ helpers
    def _require_cuda(self):
        if self._flat is None or self._flat.device.type != "cuda":
            raise L.CarelError("DrlClassifier parameters are on %s; call .to('cuda') first -- the HIP kernels are the only "
                               "implementation of the step path (no CPU fallback)." % (None if self._flat is None else self._flat.device))

    def _versions(self):
        aprx = set(self._aprx_names) | set(self._disc_names)   # fp32 only: an update of the approximation net / adversaries never stales the bf16 shadow
        return sum(p._version for k, p in self._named.items() if k not in aprx)

    def _refresh_shadow(self):
        vers = self._versions()
        if self._shadow_versions != vers:
            L.check(L.load().carel_cast_f32_to_bf16(self._flat.data_ptr(), self._shadow.data_ptr(), self._flat.numel(),
                                                    L.current_stream()), "carel_cast_f32_to_bf16")
            self._shadow_versions = vers

    def mark_shadow_fresh(self):
        """Called by the fused optimiser, which rewrites the bf16 shadow itself."""
        self._shadow_versions = self._versions()

    def _weights_ready(self):
        """Before an encoder pass: wait for weight updates still in flight on the auxiliary stream, bring the bf16 shadow up to date."""
        if self._adam_hook is not None:
            self._adam_hook._join()
        self._refresh_shadow()

    def _cached(self, key, make):
        """The small per-shape buffer stored under `key` in self._ws, built by make() on first use."""
        buf = self._ws.get(key)
        if buf is None:
            buf = self._ws[key] = make()
        return buf

    def _w(self, key, bf16=False):
        off = self._offs[key]
        base = self._shadow if bf16 else self._flat
        return base.data_ptr() + off * (2 if bf16 else 4)

    def _g(self, key):
        return self._flat_grad.data_ptr() + self._offs[key] * 4

    def _layer_arrays(self):
        if self._layer_structs is not None:
            return self._layer_structs
        n = self.cfg.layers
        P, G = (L.LayerParams * n)(), (L.LayerGrads * n)()
        for l in range(n):
            p = f"encoder.encoder.layer.{l}."
            m = dict(qkv_w=p + "attention.self.query.weight", qkv_b=p + "attention.self.query.bias",
                     out_w=p + "attention.output.dense.weight", out_b=p + "attention.output.dense.bias",
                     ln1_g=p + "attention.output.LayerNorm.weight", ln1_b=p + "attention.output.LayerNorm.bias",
                     ffn1_w=p + "intermediate.dense.weight", ffn1_b=p + "intermediate.dense.bias",
                     ffn2_w=p + "output.dense.weight", ffn2_b=p + "output.dense.bias",
                     ln2_g=p + "output.LayerNorm.weight", ln2_b=p + "output.LayerNorm.bias")
            for f, k in m.items():
                setattr(P[l], f, self._w(k, bf16=f.endswith("_w")))
                setattr(G[l], f, self._g(k))
        self._layer_structs = (P, G)
        return self._layer_structs

    def _layer_arrays_f32(self):
        """carel_layer_params with every weight pointing into the fp32 master buffer (carel_encoder_forward_f32)."""
        P, _ = self._layer_arrays()
        n = self.cfg.layers
        F = (L.LayerParams * n)()
        for l in range(n):
            for f, _t in L.LayerParams._fields_:
                setattr(F[l], f, getattr(P[l], f))
            p = f"encoder.encoder.layer.{l}."
            for f, k in dict(qkv_w="attention.self.query.weight", out_w="attention.output.dense.weight", ffn1_w="intermediate.dense.weight",
                             ffn2_w="output.dense.weight").items():
                setattr(F[l], f, self._w(p + k))
        return F

    def _run_encoder_fp32(self, c):
        """The fp32 debug forward: returns the final hidden states f32 [Bp*S, 768] (dense rows)."""
        lib = L.load()
        dev = self._flat.device
        buf = self._cached(("f32", c.Bp, c.S), lambda: SimpleNamespace(
            work=torch.zeros(lib.carel_encoder_f32_work_bytes(c.Bp, c.S), device=dev, dtype=torch.uint8),
            x=torch.zeros((c.Bp * c.S, H), device=dev, dtype=torch.float32),
            dummy=SimpleNamespace(act=torch.zeros(256, device=dev, dtype=torch.uint8), scratch=None)))
        ea =self._encoder_args(c.ids, c.att, c.tt, buf.dummy, c.Bp, c.S, True, False, 0, 0, None, None)
        F = self._layer_arrays_f32()
        ea.layers = C.cast(F, C.POINTER(L.LayerParams))
        L.check(lib.carel_encoder_forward_f32(C.byref(ea), buf.work.data_ptr(), buf.x.data_ptr(), L.current_stream()), "carel_encoder_forward_f32")
        ea._keep = F
        return ea, buf.x

    def _workspace(self, B, S, inference):
        key = (B, S, bool(inference))
        ws = self._enc_ws.get(key)
        if ws is not None:
            self._enc_ws[key] = self._enc_ws.pop(key)             # most recently used last
        if ws is None:
            # encoder activations / scratch are GBs at B = 64: keep the four most recent (batch, seq, mode) shapes -- e.g. the
            # training batch, the odd last batch and the evaluation chunk -- and drop only the least recently used one
            while len(self._enc_ws) >= 4:
                self._enc_ws.pop(next(iter(self._enc_ws)))
            lib = L.load()
            dev = self._flat.device
            ws = SimpleNamespace()
            # zero-filled once: with token packing, attention tiles read (masked) rows past a sample's last token, and
            # 0 * NaN from never-written memory would poison the MFMA sums; everything written later is finite
            ws.act = torch.zeros(lib.carel_encoder_act_bytes(B, S, self.cfg.layers, int(inference)), device=dev, dtype=torch.uint8)
            ws.scratch = torch.zeros(lib.carel_encoder_scratch_bytes(B, S), device=dev, dtype=torch.uint8)
            self._enc_ws[key] = ws
        return ws

    def _cls_info(self, B, Bp, S, pack, dev):
        """Index arrays of the dead-row elimination (include/carel_hip.h, carel_encoder_args.n_cls); B real samples,
        Bp = batch the encoder runs (padded so that Bp*S is a multiple of 128)."""
        if not self.cls_only_last or self.adapter != "false":        # an adapter reads every row of the last layer
            return None
        n_cls = (Bp + 127) // 128 * 128

        def make():
            orig = np.full(n_cls, -1, dtype=np.int32)
            orig[:B] = np.arange(B, dtype=np.int32) * S
            return SimpleNamespace(orig=torch.from_numpy(orig).to(dev), compact=torch.arange(B, dtype=torch.int32, device=dev))
        base = self._cached(("cls", B, Bp, S), make)
        if pack is None:
            rows = base.orig                      # dense: the [CLS] token of sample i sits at row i*S
        else:
            rows = torch.full((n_cls,), -1, dtype=torch.int32, device=dev)
            rows[:B] = pack.cu[:B]
        return SimpleNamespace(n_cls=n_cls, rows=rows, orig=base.orig, compact=base.compact)

    def _encoder_args(self, ids, att, tt, ws, B, S, inference, train, seed, row_offset, pack=None, cls=None):
        a = L.EncoderArgs()
        if pack is not None:
            a.n_tokens, a.tok_row, a.cu_seqlens = pack.n_tokens, pack.tok_row.data_ptr(), pack.cu.data_ptr()
        if cls is not None:
            a.n_cls, a.cls_rows, a.cls_orig_rows = cls.n_cls, cls.rows.data_ptr(), cls.orig.data_ptr()
        a.overlap_wgrad = (1 if self.overlap_wgrad else 0) | (2 if (self.overlap_wgrad and self.forward_chains) else 0)
        c = self.cfg
        a.batch, a.seq_len, a.n_layers, a.hidden, a.heads, a.intermediate = B, S, c.layers, H, NH, I_FF
        a.vocab_size, a.max_pos, a.type_vocab, a.roberta, a.pad_id, a.inference = (c.vocab_size, c.max_pos, c.type_vocab,
                                                                                      c.roberta, c.pad_id, int(inference))
        a.ln_eps = c.ln_eps
        a.hidden_dropout = c.hidden_dropout if train else 0.0
        a.attn_dropout = c.attn_dropout if train else 0.0
        a.drop_seed, a.drop_row_offset = seed, row_offset
        a.input_ids, a.attention_mask = ids.data_ptr(), (None if att is None else att.data_ptr())
        a.token_type_ids = None if tt is None else tt.data_ptr()
        e = "encoder.embeddings."
        a.word_emb, a.pos_emb, a.type_emb = self._w(e + "word_embeddings.weight"), self._w(e + "position_embeddings.weight"), self._w(e + "token_type_embeddings.weight")
        a.emb_ln_g, a.emb_ln_b = self._w(e + "LayerNorm.weight"), self._w(e + "LayerNorm.bias")
        P, G = self._layer_arrays()
        a.layers = C.cast(P, C.POINTER(L.LayerParams))
        a.layer_grads = C.cast(G, C.POINTER(L.LayerGrads))
        a.act = ws.act.data_ptr()
        a.scratch = None if ws.scratch is None else ws.scratch.data_ptr()
        a.d_word_emb, a.d_pos_emb, a.d_type_emb = self._g(e + "word_embeddings.weight"), self._g(e + "position_embeddings.weight"), self._g(e + "token_type_embeddings.weight")
        a.d_emb_ln_g, a.d_emb_ln_b = self._g(e + "LayerNorm.weight"), self._g(e + "LayerNorm.bias")
        if getattr(c, "rel_pos", False):
            span = rel_span(S)
            r = self._rel_buffers(int(a.batch), span)
            lib = L.load()
            L.check(lib.carel_relpos_expand_span(self._w(REL_KEY), r.bucket.data_ptr(), r.dist.data_ptr(), span, L.current_stream()),
                    "carel_relpos_expand_span")
            a.rel_bias_dist, a.d_rel_bias_dist = r.dist.data_ptr(), r.ddist.data_ptr()
        return a

    def _rel_buffers(self, batch=1, span=256):
        """MPNet relative positions: bucket[i] = relative_position_bucket(i - (span/2 - 1)) with the expression of transformers
        MPNetEncoder.relative_position_bucket (num_buckets 32, max_distance 128), the bias by distance [12, span] made from the
        learned table before every forward, and the gradient by distance, one row per (sample, head), that the attention backward
        kernels add into without atomics (bit-reproducible; carel_relpos_reduce_span sums the samples in order).  span 256 for S <= 128,
        1024 for the long-sequence kernels (rel_span)."""
        cache = getattr(self, "_rel_by_span", None)
        if cache is None:
            cache = self._rel_by_span = {}
        r = cache.get(span)
        dev = self._flat.device
        if r is None or r.bucket.device != dev:
            r = cache[span] = SimpleNamespace(bucket=mpnet_bucket_by_distance(span).to(dev).contiguous(),
                                              dist=torch.zeros((NH, span), device=dev, dtype=torch.float32),
                                              ddist=torch.zeros((NH, span), device=dev, dtype=torch.float32))
        if r.ddist.shape[0] < batch * NH:
            r.ddist = torch.zeros((batch * NH, span), device=dev, dtype=torch.float32)
        return r

    @staticmethod
    def _prep_ids(t, Bp, Sp=None, fill=0):
        """[B, S] -> [Bp, Sp] int64: zero rows below (filler samples), `fill` columns on the right (positions that pad the length up
        to a multiple of 32: token ids get pad_id, the attention mask 0)."""
        t = t.to(torch.long).contiguous()
        if Sp is not None and t.shape[1] != Sp:
            t = torch.cat((t, torch.full((t.shape[0], Sp - t.shape[1]), fill, dtype=t.dtype, device=t.device)), dim=1)
        if t.shape[0] != Bp:
            pad = torch.zeros((Bp - t.shape[0], t.shape[1]), dtype=t.dtype, device=t.device)
            t = torch.cat((t, pad), dim=0)
        return t

    @staticmethod
    def _padded_len(S, max_pos=512, roberta=0, pad_id=0, adapter="false"):
        """The length the encoder runs for inputs of S positions: S rounded up to a multiple of 32, at most 512 and at most the rows of
        the position table (BERT: max_pos; RoBERTa / MPNet, whose ids start at pad_id + 1: max_pos - pad_id - 1).  The extra positions
        are masked: a masked key contributes exactly zero and the packed path skips it, so every result equals a run at the rounded
        length.  Sentence adapters attend to padding too: they keep S in {32, 64, 96, 128}."""
        limit = min(512, max_pos - pad_id - 1 if roberta else max_pos)
        if S < 1 or S > limit:
            raise L.CarelError("sequence length must be at most %d (--max_len; the position table has %d rows%s); got %d"
                               % (limit, max_pos, ", ids from pad_id + 1" if roberta else "", S))
        Sp = (S + 31) // 32 * 32
        if adapter not in ("false", False, None) and (Sp != S or S > 128):
            raise L.CarelError("with a sentence adapter the sequence length must be 32, 64, 96 or 128 (--max_len; adapters attend to "
                               "padded positions); got %d" % S)
        return Sp

    def _padded_shape(self, B, S):
        """(Bp, Sp): the batch and length the encoder runs (_padded_len, _padded_batch) for this model."""
        c = self.cfg
        Sp = self._padded_len(S, c.max_pos, c.roberta, c.pad_id, getattr(self, "adapter", "false"))
        return self._padded_batch(B, Sp), Sp

    @staticmethod
    def _padded_batch(B, S):
        if S < 32 or S > 512 or S % 32:
            raise L.CarelError("sequence length must be a multiple of 32 in [32, 512] (--max_len); got %d" % S)
        Bp = B
        while (Bp * S) % 128:
            Bp += 1
        return Bp

    def _pack_info(self, att, B, Bp, S, seq_lengths=None):
        """Token packing for padded batches: only attended positions go through the encoder (the reference pads every
        pair to max_len and ~77 % of ECPE tokens are padding).  Exact for prefix-form masks (HF right padding): padded
        positions are never attended to and nothing but [CLS] is read from the last layer, so every output and
        gradient is unchanged; dropout masks and position ids keep using the ORIGINAL (sample, position) index.
        Returns None to run dense (no padding in the batch, non-prefix mask, or varlen disabled; always with a sentence adapter, which
        attends to the padded positions too)."""
        if not self.varlen or att is None or self.adapter != "false":
            return None
        if seq_lengths is None:
            m = att[:B].to(torch.int32)
            lens = m.sum(1)
            prefix = ((torch.arange(S, device=m.device)[None, :] < lens[:, None]).to(torch.int32) == m).all()
            info = torch.cat((lens, prefix.to(torch.int32).reshape(1))).cpu()        # the one host sync of the packed path
            lens_l, ok = info[:-1].tolist(), bool(info[-1])
        else:
            lens_l, ok = [int(v) for v in seq_lengths], True
        if not ok or min(lens_l) < 1:
            return None
        t_eff = sum(lens_l)
        if t_eff == B * S:
            return None
        if getattr(seq_lengths, "cu", None) is not None and seq_lengths.t_eff == t_eff and seq_lengths.cu.numel() == Bp + 1:
            # carel_vae_amd.data.PrefetchLoader shipped the packing arrays with the batch: nothing to build or copy here
            return SimpleNamespace(n_tokens=seq_lengths.n_tokens, t_eff=t_eff, cu=seq_lengths.cu, tok_row=seq_lengths.tok_row)
        t_pad = (t_eff + 127) // 128 * 128
        lens_a = np.asarray(lens_l, dtype=np.int64)
        cu = np.zeros(Bp + 1, dtype=np.int32)
        cu[1:B + 1] = np.cumsum(lens_a)
        cu[B + 1:] = t_eff
        tok = np.full(t_pad, -1, dtype=np.int32)
        starts = np.repeat(np.arange(B, dtype=np.int64) * S - cu[:B], lens_a)
        tok[:t_eff] = (np.arange(t_eff, dtype=np.int64) + starts).astype(np.int32)
        dev = att.device
        return SimpleNamespace(n_tokens=t_pad, t_eff=t_eff, cu=torch.from_numpy(cu).to(dev, non_blocking=True),
                               tok_row=torch.from_numpy(tok).to(dev, non_blocking=True))

    def _prepare_inputs(self, input_ids, att_masks, token_type_ids, seq_lengths=None):
        """How a batch gets to the encoder, for every model path: a call record with B (real samples), S and Bp (the length and batch the
        encoder runs: _padded_shape), ids / att / tt padded to [Bp, S] (_prep_ids) and the token packing (_pack_info; None = dense).
        Works on the tensors' own device; with seq_lengths given nothing is read back."""
        c = _Call()
        c.B, S = input_ids.shape
        c.Bp, c.S = self._padded_shape(c.B, S)
        c.ids, c.att = self._prep_ids(input_ids, c.Bp, c.S, self.cfg.pad_id), self._prep_ids(att_masks, c.Bp, c.S)
        c.tt = None if token_type_ids is None else self._prep_ids(token_type_ids, c.Bp, c.S)
        c.pack = self._pack_info(c.att, c.B, c.Bp, c.S, seq_lengths)
        return c

    def _run_encoder(self, c, training, train_drop, seed, row_offset, want_cls=True, weights_ready=False):
        """The one bf16 encoder pass over a prepared record (_prepare_inputs): records c.ws, c.cls (the [CLS] compaction; None without
        want_cls or where _cls_info declines) and c.ea, and returns (x_last_ptr, cls_rows, n_rows): where a reader of the last layer
        finds sample i -- compact [CLS] rows, else the packed sample starts, else dense (None: row i*S) -- and how many rows there are.
        weights_ready: the caller has brought the bf16 shadow up to date itself (the chunk loops do it once, before the first chunk)."""
        if not weights_ready:
            self._weights_ready()
        lib = L.load()
        c.ws = self._workspace(c.Bp, c.S, inference=not training)
        c.cls = self._cls_info(c.B, c.Bp, c.S, c.pack, self._flat.device) if want_cls else None
        c.ea = self._encoder_args(c.ids, c.att, c.tt, c.ws, c.Bp, c.S, not training, train_drop, seed, row_offset, c.pack, c.cls)
        L.check(lib.carel_encoder_forward(C.byref(c.ea), L.current_stream()), "carel_encoder_forward")
        x_last_ptr = lib.carel_encoder_x_last(C.byref(c.ea))
        if c.cls is not None:
            return x_last_ptr, c.cls.compact, c.cls.n_cls
        if c.pack is not None:
            return x_last_ptr, c.pack.cu, c.pack.n_tokens
        return x_last_ptr, None, c.Bp * c.S

    def _next_seed(self):
        """The dropout seed of the next forward call (every mask of one call derives from it)."""
        self._fwd_count += 1
        return (self.dropout_base_seed * 1000003 + self._fwd_count) & 0xFFFFFFFF

    def _tail_buffers(self, c):
        return self._cached(("tail", c.B, c.S), lambda: ops.TailBuffers(c.B, c.S, self.opt.ec_dim, self.opt.e_num_class, self.opt.pair_bow_dim,
                                                                        c.ids.device, rows=c.Bp * c.S))

    @contextlib.contextmanager
    def _overwriting_grads(self, accumulate, lo=0, hi=None, keep=()):
        """Around a backward that overwrites [lo, hi) of the flat gradient buffer (default: all of it).  accumulate: the caller's answer
        to "do these parameters already hold a gradient?"; then what the range held is set aside and added back afterwards, as
        autograd accumulates.  keep: (klo, khi) sub-ranges that the backward leaves alone or accumulates into by itself, which must not
        be added to themselves.  Yields accumulate; the caller binds the .grad views when the block is done."""
        prev = None
        if accumulate:
            prev = self._flat_grad[lo:hi].clone()
            for klo, khi in keep:
                prev[klo - lo:khi - lo].zero_()
        yield accumulate
        if accumulate:
            self._flat_grad[lo:hi].add_(prev)

    def set_noise(self, eps_e, eps_c):
        """Test hook: use these two [ec_dim] vectors as the next call's reparameterisation noise (ref :350)."""
        self._noise = None if eps_e is None else (eps_e, eps_c)

    def _draw_noise(self, dev):
        if self._noise is not None:
            e, c = self._noise
            self._noise = None
            return e.to(dev, torch.float32).contiguous(), c.to(dev, torch.float32).contiguous()
        D = self.opt.ec_dim
        if self._dp is not None:                     # same draws on every rank, no collective
            return self._dp.draw_noise(D, dev)
        eps_e = torch.randn(D, device=dev)           # emotion first, then cause (ref :215-216)
        eps_c = torch.randn(D, device=dev)
        return eps_e, eps_c

    # ------------------------------------------------------------------ forward / backward bodies
    def _make_call(self, input_ids, att_masks, token_type_ids, emotion_labels, cause_labels, pair_labels, content_bow, iteration, training,
                   seq_lengths=None):
        self._require_cuda()
        ops._chk_cuda(input_ids, att_masks, token_type_ids, content_bow)
        B = input_ids.shape[0]
        self._padded_shape(*input_ids.shape)         # a length the encoder refuses is refused before anything is drawn or counted
        dev = input_ids.device
        f32 = torch.float32
        labels = dict(emo=emotion_labels.to(dev, torch.long).reshape(-1).contiguous(), cau=cause_labels.to(dev, f32).reshape(-1).contiguous(),
                      pair=pair_labels.to(dev, f32).reshape(-1).contiguous(), bow=content_bow.to(dev, f32).contiguous())
        if labels["bow"].shape != (B, self.opt.pair_bow_dim):
            raise L.CarelError("content_bow must be [batch, pair_bow_dim]")
        eps = self._draw_noise(dev)
        seed = self._next_seed()
        # after the launches above: the packing arrays go to the device in host-to-device copies, which the host may have to wait for
        c = self._prepare_inputs(input_ids, att_masks, token_type_ids, seq_lengths)
        c.labels, c.iteration, c.training, c.seed = labels, int(iteration), training, seed
        c.eps_e, c.eps_c = eps
        c.row_offset = 0 if self._dp is None else self._dp.row_offset(B)
        if self.adapter != "false" and self._dp is not None:
            raise L.CarelError("sentence adapters are not supported under DataParallel")
        if self._gan:
            if self._dp is not None:
                raise L.CarelError("opt.disentangle == 'gan' is not supported under DataParallel")
            c.labels["emo_f"] = emotion_labels.to(dev, f32).reshape(-1).contiguous()     # the adversaries score float labels (:83, :133)
            if c.labels["emo_f"].numel() != B or c.labels["cau"].numel() != B:
                raise L.CarelError("emotion_labels and cause_labels must hold one value per pair")
        self._check_tail_batch(B)
        c.buf = self._tail_buffers(c)
        if self._dp is not None:
            self._dp.prepare(c)
        return c

    def _check_tail_batch(self, B):
        """The combinations the loss step refuses, raised when the batch is known and before the encoder runs: above the
        single-workgroup limit of carel_tail_losses the batch-tiled form takes over (ops.tail_losses), which has MMD or no statistic
        (vi and gan add theirs beside it, within their own kernels' limits) and at most 1024 rows."""
        limit = ops.tail_batch_limit(self.opt.ec_dim, self.opt.e_num_class)
        if B <= limit:
            return
        if getattr(self.opt, "disentangle", "mmd") == "hsic":
            raise L.CarelError("opt.disentangle == 'hsic' keeps the single-workgroup tail: batch <= %d per GPU at ec_dim %d; got %d "
                               "(the other disentanglers train up to 1024 per GPU)" % (limit, self.opt.ec_dim, B))
        if B > 1024:
            raise L.CarelError("the loss step takes at most 1024 pairs per GPU (--batch_size); got %d" % B)

    def _tail_weights(self):
        keys = ["encoder.pooler.dense.weight", "encoder.pooler.dense.bias", "decoder.weight", "decoder.bias"]
        for n in ("emotion_mu", "emotion_log_var", "cause_mu", "cause_log_var", "emotion_classifier", "cause_classifier", "pair_classifier"):
            keys += [n + ".weight", n + ".bias"]
        lo, hi = self._head_range            # the loss kernels' outputs go to the image (_flatten), the backward's into .grad
        return ({k: self._named[k].data for k in keys},
                {k: self._head_img_view(k) if lo <= self._offs[k] < hi else self._grad_view(k) for k in keys})

    def _grad_view(self, k):
        p = self._named[k]
        o = self._offs[k]
        return self._flat_grad[o:o + p.numel()].view(p.shape)

    # ------------------------------------------------------------------ sentence adapters (EMNLP scripts)
    def _adapter_weights(self):
        out = []
        for side in ("emotion", "cause"):
            m = getattr(self, side + "_adapter")
            if self.adapter == "raw":
                w, b = m.in_proj_weight.data, m.in_proj_bias.data
                out.append(dict(q_w=w[:H], q_b=b[:H], k_w=w[H:2 * H], v_w=w[2 * H:], v_b=b[2 * H:], o_w=m.out_proj.weight.data,
                                o_b=m.out_proj.bias.data))
            else:
                out.append(dict(q_w=m.q_proj.weight.data, q_b=m.q_proj.bias.data, k_w=m.k_proj.weight.data))
        return out

    def _adapter_grads(self):
        """The destinations of carel_adapter_backward_weights in the flat gradient buffer, keyed like _adapter_weights() with a d_ prefix."""
        out = []
        for side in ("emotion", "cause"):
            g = lambda n: self._grad_view("%s_adapter.%s" % (side, n))        # noqa: E731
            if self.adapter == "raw":
                w, b = g("in_proj_weight"), g("in_proj_bias")
                out.append(dict(d_q_w=w[:H], d_q_b=b[:H], d_k_w=w[H:2 * H], d_k_b=b[H:2 * H], d_v_w=w[2 * H:], d_v_b=b[2 * H:],
                                d_o_w=g("out_proj.weight"), d_o_b=g("out_proj.bias")))
            else:
                out.append(dict(d_q_w=g("q_proj.weight"), d_q_b=g("q_proj.bias"), d_k_w=g("k_proj.weight"), d_k_b=g("k_proj.bias")))
        return out

    def _adapter_forward(self, c, x_last_ptr):
        """Adapter outputs [2, B, 768] from the dense last hidden states.  u is rebuilt on every call (a few microseconds), so a change
        of the queries or adapter weights by any route -- load_state_dict, an in-place edit, a write through .data -- takes effect."""
        dev = self._flat.device
        G = self.head_number if self.adapter == "raw" else 1
        buf = self._cached(("adapter", c.B, c.S), lambda: ops.AdapterBuffers(c.B, c.S, G, dev))
        qs = [getattr(self, n).to(dev, torch.float32).reshape(-1).contiguous() for n in ("emotion_q", "cause_q")]
        if qs[0].numel() != H or qs[1].numel() != H:
            raise L.CarelError("emotion_q / cause_q must hold 768 values")
        u = self._cached("adapter_u", lambda: torch.empty((2, G, H), device=dev, dtype=torch.float32))
        a = ops.adapter_args(self.adapter, G, qs, self._adapter_weights(), u, buf, c.Bp, x=SimpleNamespace(data_ptr=lambda: x_last_ptr))
        ops.adapter_build_u(a)
        ops.adapter_forward(a)
        return a, buf

    def _run_forward(self, c, training):
        train_drop = self.training          # dropout follows module mode (model.train() / .eval()), like nn.Dropout
        if self.debug_fp32:
            self._weights_ready()
            if training:
                raise L.CarelError("debug_fp32 is a forward-only measurement mode: call forward_terms() / forward() under torch.no_grad()")
            train_drop = False
            c.pack, c.cls, c.ws = None, None, None
            c.ea, x_f32 = self._run_encoder_fp32(c)
            x_last_ptr, cls_rows, n_rows = x_f32.data_ptr(), None, c.Bp * c.S
        else:
            x_last_ptr, cls_rows, n_rows = self._run_encoder(c, training, train_drop, c.seed, c.row_offset)
        W, G = self._tail_weights()
        xl = SimpleNamespace(data_ptr=lambda: x_last_ptr)
        c.ad = None
        head_in = d_head_in = None
        if self.adapter != "false":
            c.ad, abuf = self._adapter_forward(c, x_last_ptr)
            head_in, d_head_in = abuf.out, abuf.d_out
        klw = ops.kl_anneal_weight(c.iteration, self.opt)
        drop = (self.opt.dropout if train_drop else 0.0, c.seed, c.row_offset)
        ta = ops.tail_args(c.buf, xl, W, c.labels, c.eps_e, c.eps_c, self.opt, klw, grads=G, drop=drop, cls_rows=cls_rows, n_rows=n_rows,
                           head_in=head_in, d_head_in=d_head_in)
        ops.tail_latents(ta)
        if self._dp is not None:
            self._dp.fill_global(ta, c)                  # all-gather z, all-reduce label sum
        ta.serial = 0 if self.overlap_wgrad else 1       # side stream allowed: the loss kernel runs beside the decoder passes
        ops.tail_losses(ta)
        if self._gan:                                    # the two adversaries on the z the tail has written; terms[4] = the script's vae loss
            c.gan_terms = self._gan_disc(c, drop)
        c.ta = ta
        c.keep = (W, G, xl)

    def _gan_disc(self, c, drop):
        terms = self._cached(("gan_terms", c.B, c.S), lambda: torch.zeros(8, device=self._flat.device, dtype=torch.float32))

        def img(i, k):
            o = self._offs[k] - self._disc_lo
            return self._disc_img[i][o:o + self._named[k].numel()]
        w = [self._named[g + ".weight"].data for g in GAN_DISCS]
        b = [self._named[g + ".bias"].data for g in GAN_DISCS]
        ops.gan_disc(c.buf.z, c.labels["emo_f"], c.labels["cau"], w, b, self.opt, terms,
                     [img(0, g + ".weight") for g in GAN_DISCS], [img(0, g + ".bias") for g in GAN_DISCS],
                     [img(1, g + ".weight") for g in GAN_DISCS], [img(1, g + ".bias") for g in GAN_DISCS],
                     drop=drop, vae_loss_in=c.buf.terms[8:9])
        return terms

    def _group_has_grad(self, g):
        """Does a backward call into group g accumulate?  An adversary's range is written as a whole, so both of its parameters count:
        it accumulates only when both hold a gradient (as FusedRMSprop.step steps only then); a half-cleared group is overwritten."""
        if g == "vae":
            return self._named["encoder.embeddings.word_embeddings.weight"].grad is not None
        return all(self._named[g + t].grad is not None for t in (".weight", ".bias"))

    def _run_backward_gan(self, c, grads):
        """Backward of the (ec_disc_loss, ce_disc_loss, vae_and_classifier_loss) tuple (drl_classifier_ec_gan.py:784-802): a
        discriminator loss adds its own image, scaled by its upstream gradient, into that discriminator's .grad; the vae loss runs the
        encoder backward and adds ecce_adv_loss_weight x the entropy image into BOTH discriminators' .grad -- accumulating like torch."""
        f32 = torch.float32
        if self._grad_views is None:
            self._grad_views = {k: self._grad_view(k) for k in self._order}

        def share(group, image, g_dev):
            lo, hi = self._group_ranges[group]
            ops.axpy_(self._flat_grad[lo:hi], self._disc_img[image][lo - self._disc_lo:hi - self._disc_lo], g_dev, self._group_has_grad(group))
            for t in (".weight", ".bias"):
                self._named[group + t].grad = self._grad_views[group + t]

        for i, group in enumerate(GAN_DISCS):
            if grads[i] is not None:
                share(group, 0, grads[i].to(f32).reshape(1).contiguous())
        if grads[2] is not None:
            go = grads[2].to(f32).reshape(1).contiguous()
            w = float(self.opt.ecce_adv_loss_weight)
            ge = go if w == 1.0 else go * w
            for group in GAN_DISCS:
                share(group, 1, ge)
            self._run_backward(c, go, None)

    def _run_backward(self, c, grad_out, grad_z=None):
        # the adversaries' range (gan) and the approximation network's (vi: _AprxLoss.backward owns it; the tail of the flat buffer) are
        # not rewritten below, and the classifier / decoder range accumulates by itself: they must not be added to themselves
        keep = [self._head_range]
        if self._gan:
            keep.append((self._disc_lo, self._disc_hi))
        if self._aprx_names:
            keep.append((self._offs[self._aprx_names[0]], self._flat_grad.numel()))
        with self._overwriting_grads(self._group_has_grad("vae"), keep=keep) as accumulate:
            go = grad_out.to(torch.float32).reshape(1).contiguous()      # device scalar, never read on the host
            ea = c.ea
            ea.dx = c.buf.dx_last.data_ptr()          # [Bp*S (or packed n_tokens), 768]; cleared + CLS rows written by the tail backward
            ops.tail_backward(c.ta, go, None if grad_z is None else grad_z.to(torch.float32).contiguous())
            if c.ad is not None:                     # adapter mode: d head_in -> every row of dx_last (the tail left dx_last alone)
                c.ad.dx_f32 = ea.dx
                ops.adapter_backward(c.ad)
                if self._adapter_train_names:        # opt.train_adapter: overwritten like every gradient of this call
                    ops.adapter_backward_weights(c.ad, ops.adapter_wgrad_args(self._ws[("adapter", c.B, c.S)], self._adapter_grads()))
            # classifier / decoder gradients were produced by the forward for grad_output = 1, as an image of one contiguous range
            lo, hi = self._head_range
            ops.axpy_(self._flat_grad[lo:hi], self._head_img, go, accumulate)
            if self._dp is not None:
                self._dp.tail_done()
            self._backward_encoder(ea, accumulate)
            if c.ad is not None:
                # the adapters read padded positions, so for once they carry gradient; HF's embeddings have padding_idx = pad_id (word table,
                # and RoBERTa's position table, whose padded positions take position pad_id): that row gets none
                e = "encoder.embeddings."
                self._grad_view(e + "word_embeddings.weight")[self.cfg.pad_id].zero_()
                if self.cfg.roberta:
                    self._grad_view(e + "position_embeddings.weight")[self.cfg.pad_id].zero_()
            if self._dp is not None:
                self._dp.backward_done(None if accumulate else self._adam_hook)
        self._bind_grads()
        if self.strict_pair_skip and self._has_pair_skip and not accumulate:
            # stock optimisers: leave pair_classifier.grad None when the pair loss was replaced by 0, exactly as the reference
            # does (:510-511) -- torch.optim.Adam then skips the parameter.  One device->host read per step (the reference's
            # own `if torch.isinf(...).any()` is such a read too); FusedAdam needs no read (carel_adam_args.skip_flag).
            off = L.load().carel_tail_pair_dead_offset(c.B, self.opt.ec_dim, self.opt.pair_bow_dim)
            if float(c.buf.work[off]) != 0.0:
                for k in self._pair_range_names:
                    self._named[k].grad = None

    def _backward_encoder(self, ea, accumulate):
        """Encoder layers 11..0 and the embeddings, given ea.dx = d loss / d (last hidden states)."""
        lib = L.load()
        st = L.current_stream()

        def layer_ready(l):             # layer l's parameter gradients are complete in the order of the main stream
            work = self._dp.layer_done(l) if self._dp is not None else None
            if self._adam_hook is not None and not accumulate and (self._dp is None or work is not None):
                self._adam_hook._layer_ready(l, after=work)

        span = rel_span(int(ea.seq_len))
        rel = self._rel_buffers(int(ea.batch), span) if getattr(self.cfg, "rel_pos", False) else None
        if rel is not None:
            if rel.ddist.data_ptr() != ea.d_rel_bias_dist:
                raise L.CarelError("internal: the relative-position gradient buffer was re-allocated between forward and backward")
            rel.ddist[:int(ea.batch) * NH].zero_()
        lag = 1 if self.overlap_wgrad else 0     # with the side stream a layer completes one call late (include/carel_hip.h)
        for l in range(self.cfg.layers - 1, -1, -1):
            L.check(lib.carel_encoder_backward_layer(C.byref(ea), l, st), "carel_encoder_backward_layer")
            if l + lag < self.cfg.layers:
                layer_ready(l + lag)
        if lag:
            L.check(lib.carel_encoder_backward_join(C.byref(ea), st), "carel_encoder_backward_join")
            layer_ready(0)
        L.check(lib.carel_encoder_backward_embeddings(C.byref(ea), st), "carel_encoder_backward_embeddings")
        if rel is not None:      # fold the gradient by distance (every layer's attention backward added to it) into the table's buckets
            L.check(lib.carel_relpos_reduce_span(rel.ddist.data_ptr(), int(ea.batch), rel.bucket.data_ptr(), self._g(REL_KEY), 0, span, st),
                    "carel_relpos_reduce_span")

    def _bind_grads(self):
        if self._grad_views is None:
            self._grad_views = {k: self._grad_view(k) for k in self._order}
        skip = set(self._aprx_names) | (set(self._adapter_names) - set(self._adapter_train_names)) | set(self._disc_names)
        for k, p in self._named.items():
            if k not in skip:               # the approximation net's gradients belong to _AprxLoss.backward (the adversaries': _run_backward_gan); adapters get none (frozen) unless opt.train_adapter
                p.grad = self._grad_views[k]

    # ------------------------------------------------------------------ public API (reference surface)
    def forward(self, input_ids, att_masks, token_type_ids, emotion_labels, cause_labels, pair_labels, content_bow, iteration,
                seq_lengths=None):
        """Reference `forward` (:184-263): returns the scalar `vae_and_classifier_loss`.
        seq_lengths (optional extension): host list of attended lengths per pair; saves the device->host read that the
        padding-skipping path otherwise needs to learn them from `att_masks`."""
        c = self._make_call(input_ids, att_masks, token_type_ids, emotion_labels, cause_labels, pair_labels, content_bow, iteration,
                            training=torch.is_grad_enabled(), seq_lengths=seq_lengths)
        self._last_call = c
        vi = bool(self._aprx_names)
        D = self.opt.ec_dim
        if self._gan:            # drl_classifier_ec_gan.py:281: (ec_disc_loss, ce_disc_loss, vae_and_classifier_loss)
            if torch.is_grad_enabled():
                return _GanLosses.apply(self._flat.new_zeros((), requires_grad=True), self, c)
            self._run_forward(c, training=False)
            t = c.gan_terms
            return t[0].clone(), t[1].clone(), t[4].clone()
        if torch.is_grad_enabled():
            anchor = self._flat.new_zeros((), requires_grad=True)
            loss, z = _TrainLoss.apply(anchor, self, c)
            c.z_out = z
            if vi:          # drl_classifier_ec_vi.py:263: (sampled_emotion_emb, sampled_cause_emb, ec_aprx_loss, vae_and_classifier_loss)
                z_e, z_c = z[:, :D], z[:, D:]
                return z_e, z_c, self.get_ec_aprx_loss(z_e, z_c), loss
            return loss
        self._run_forward(c, training=False)
        loss = c.buf.terms[8].clone()
        if vi:
            z = c.buf.z.clone()
            return z[:, :D], z[:, D:], self.get_ec_aprx_loss(z[:, :D], z[:, D:]), loss
        return loss

    def sampled_embeddings(self):
        """(z_e, z_c) of the most recent training forward, connected to autograd: any extra loss term built on them
        back-propagates into the encoder together with the returned loss (extension; the VI variant returns them itself)."""
        z = self._last_call.z_out
        D = self.opt.ec_dim
        return z[:, :D], z[:, D:]

    def forward_terms(self, *args, **kw):
        """Added introspection entry point: the loss plus every term and the latent means (no autograd)."""
        with torch.no_grad():
            self.forward(*args, **kw)
        c = self._last_call
        t = c.buf.terms.clone()
        D = self.opt.ec_dim
        lat = c.buf.lat.clone()
        out = {n: t[i] for i, n in enumerate(self.TERM_NAMES)}
        out.update(mu_e=lat[:, :D], lv_e=lat[:, D:2 * D], mu_c=lat[:, 2 * D:3 * D], lv_c=lat[:, 3 * D:], z=c.buf.z.clone())
        if self._gan:            # "loss" stays the tail's own total; "vae_and_classifier_loss" adds the weighted entropies (:275-279)
            g = c.gan_terms.clone()
            out.update({n: g[i] for i, n in enumerate(ops.GAN_TERM_NAMES)})
            out["vae_and_classifier_loss"] = g[4]
        if c.ad is not None:                 # the heads' inputs: emotion / cause adapter outputs (the pooler is not run)
            a = self._ws[("adapter", c.B, c.S)].out
            out.update(adapter_e=a[0].clone(), adapter_c=a[1].clone())
        else:
            out.update(pooled=c.buf.pooled.clone())
        return out

    def last_terms(self):
        """Terms of the most recent forward (device tensor, no sync)."""
        return {n: self._last_call.buf.terms[i] for i, n in enumerate(self.TERM_NAMES)}

    def pair_probabilities(self, input_ids, att_masks, token_type_ids, chunk=1024):
        """sigmoid(pair_classifier([z_e, z_c])) with fresh noise even in eval mode (ref :277-282, quirk Q6).  The reference feeds the
        whole test set as one batch (:958); here it goes through the encoder in chunks (inference workspace: one layer's activations
        for `chunk` pairs).  Measured on 2 048 ECPE-shaped pairs (tools/bench_infer.py): 73 / 97 / 113 / 120 k pairs/s at chunks of
        128 / 256 / 512 / 1 024 -- larger GEMM grids and fewer length read-backs."""
        self._require_cuda()
        ops._chk_cuda(input_ids, att_masks, token_type_ids)
        eps_e, eps_c = self._draw_noise(input_ids.device)
        lat = self.pair_latents(input_ids, att_masks, token_type_ids, chunk=chunk)
        W, _ = self._tail_weights()
        return ops.pair_probs(lat, eps_e, eps_c, W["pair_classifier.weight"], W["pair_classifier.bias"], self.opt.ec_dim)

    def pair_latents(self, input_ids, att_masks, token_type_ids, chunk=1024):
        """The deterministic front of `pair_probabilities` (extension): eval-mode encoder in chunks, [CLS]-only last layer, pooler or
        adapters, latent heads -> lat [N, 4 * ec_dim] f32 = [mu_e | log_var_e | mu_c | log_var_c] on the device.  No noise is drawn.
        `pair_probabilities_from` / `draw_counts` then evaluate any number of noise draws on it without another encoder pass."""
        self._require_cuda()
        ops._chk_cuda(input_ids, att_masks, token_type_ids)
        N = input_ids.shape[0]
        out = torch.empty((N, 4 * self.opt.ec_dim), device=input_ids.device, dtype=torch.float32)
        self._refresh_shadow()
        for s in range(0, N, chunk):
            c = self._prepare_inputs(input_ids[s:s + chunk], att_masks[s:s + chunk], None if token_type_ids is None else token_type_ids[s:s + chunk])
            x_last_ptr, cls_rows, _ = self._run_encoder(c, False, False, 0, 0, weights_ready=True)
            buf = self._tail_buffers(c)
            W, _ = self._tail_weights()
            head_in = None
            if self.adapter != "false":
                _, abuf = self._adapter_forward(c, x_last_ptr)
                head_in = abuf.out
            ta = ops.tail_args(buf, SimpleNamespace(data_ptr=lambda: x_last_ptr), W, None, None, None, self.opt, 1.0, cls_rows=cls_rows,
                               head_in=head_in)
            ops.tail_latents(ta)
            out[s:s + c.B] = buf.lat
        return out

    def _draws_noise(self, dev, n_draws, noise):
        D = self.opt.ec_dim
        if noise is None:            # what n_draws successive forward / pair_probabilities calls draw: emotion then cause, per draw
            if int(n_draws) < 1:
                raise L.CarelError("n_draws must be >= 1")
            pairs = [self._draw_noise(dev) for _ in range(int(n_draws))]
            return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
        eps_e, eps_c = (torch.as_tensor(x).to(dev, torch.float32).reshape(-1, D).contiguous() for x in noise)
        if eps_e.shape != eps_c.shape or eps_e.shape[0] < 1:
            raise L.CarelError("noise must be (eps_e [K, ec_dim], eps_c [K, ec_dim]) with K >= 1")
        return eps_e, eps_c

    def pair_probabilities_from(self, lat, n_draws=1, noise=None, return_noise=False):
        """prob [K, N] f32: `pair_probabilities` for K noise draws on the latents of `pair_latents`, in one launch (extension).  Without
        `noise` it draws what K successive `pair_probabilities` calls draw, so row k has the bits of the k-th such call from the same
        generator state; noise = (eps_e [K, D], eps_c [K, D]) replays chosen draws (return_noise=True hands them back)."""
        self._require_cuda()
        eps_e, eps_c = self._draws_noise(lat.device, n_draws, noise)
        W, _ = self._tail_weights()
        prob, _ = ops.pair_probs_draws(lat, eps_e, eps_c, W["pair_classifier.weight"], W["pair_classifier.bias"], self.opt.ec_dim)
        return (prob, (eps_e, eps_c)) if return_noise else prob

    def latent_two_sample_test(self, lat, n_permutations=1000, noise=None, alphas=None, labels=None, generator=None, return_stats=False,
                               return_widths=False):
        """Are the emotion and the cause latents distinguishable (extension)?  The permutation two-sample test of `mmd_two_sample_test`
        on z_e, z_c [N, ec_dim] sampled from the latents of `pair_latents` the way draw 0 of `pair_probabilities_from` samples them
        (noise = (eps_e, eps_c) replays a chosen draw; without it one is drawn like a forward call's).  alphas defaults to the kernel
        width of the model's own MMD loss term; "median" takes the median heuristic of the sampled z the test then runs on (same
        noise, same call).  2 N <= 8192.  Returns (mmd, pval), with return_stats (mmd, pval, stats, count); return_widths appends
        {"alphas": the list used}."""
        _is_median("latent_two_sample_test", "alphas", alphas)
        self._require_cuda()
        D = self.opt.ec_dim
        eps_e, eps_c = self._draws_noise(lat.device, 1, noise)
        z = ops.sample_latents(lat, eps_e[0].contiguous(), eps_c[0].contiguous(), D)
        return mmd_two_sample_test(z[:, :D], z[:, D:], ops.MODEL_MMD_ALPHAS if alphas is None else alphas, n_permutations, eps=1e-5,
                                   labels=labels, generator=generator, return_stats=return_stats, return_widths=return_widths)

    def latent_independence_test(self, lat, n_permutations=1000, noise=None, s_e=1.0, s_c=1.0, permutations=None, generator=None,
                                 return_stats=False, return_widths=False):
        """Are the emotion and the cause latent of the same pair independent (extension)?  The permutation independence test of
        `hsic_independence_test` on z_e, z_c [N, ec_dim] sampled from the latents of `pair_latents` exactly as
        `latent_two_sample_test` samples them (noise = (eps_e, eps_c) replays a chosen draw; without it one is drawn like a forward
        call's).  s_e, s_c: the kernel widths of the two Gram matrices; "median" takes the median heuristic of the sampled z_e / z_c
        the test then runs on (same noise, same call).  N <= 8192.  Returns (hsic, pval), with return_stats (hsic, pval, stats,
        count); return_widths appends {"s_e": ..., "s_c": ...}, the widths used."""
        _is_median("latent_independence_test", "s_e", s_e), _is_median("latent_independence_test", "s_c", s_c)
        self._require_cuda()
        D = self.opt.ec_dim
        eps_e, eps_c = self._draws_noise(lat.device, 1, noise)
        z = ops.sample_latents(lat, eps_e[0].contiguous(), eps_c[0].contiguous(), D)
        out = hsic_independence_test(z[:, :D], z[:, D:], s_e, s_c, n_permutations, permutations=permutations, generator=generator,
                                     return_stats=return_stats, return_widths=return_widths)
        return out[:-1] + (dict(s_e=out[-1]["s_x"], s_c=out[-1]["s_y"]),) if return_widths else out

    def draw_counts(self, lat, labels, n_draws, groups=None, noise=None, return_noise=False, n_groups=None):
        """int64 [K, G, 3]: TP / FP / FN of `prob > 0.5` (numpy's .round() of a probability, ref :282: exactly 0.5 predicts 0) against
        `labels == 1`, per noise draw and group, without materialising the [K, N] probabilities (extension; the case analysis'
        re-evaluation loop, mmd_wommd_case_analysis.py:662-696).  groups: int [N] ids in [0, G), G <= 8 (default: one group);
        n_groups: G when the highest id is unused (default max id + 1).  The overall counts are the sum over groups."""
        self._require_cuda()
        dev = lat.device
        N = lat.shape[0]
        labels = torch.as_tensor(labels).to(dev, torch.float32).reshape(-1).contiguous()
        if labels.numel() != N:
            raise L.CarelError("draw_counts: one label per row of lat")
        G = 1 if n_groups is None else int(n_groups)
        if groups is not None:
            groups = torch.as_tensor(groups).reshape(-1)
            if groups.numel() != N or groups.dtype.is_floating_point:
                raise L.CarelError("draw_counts: groups must be N integer ids")
            lo, hi = int(groups.min()), int(groups.max())           # checked on the host before any launch
            if n_groups is None:
                G = hi + 1
            if lo < 0 or hi >= G:
                raise L.CarelError("draw_counts: group ids must be in [0, %d)" % G)
            groups = groups.to(dev, torch.int32).contiguous()
        if not 1 <= G <= ops.PAIR_DRAWS_MAX_GROUPS:
            raise L.CarelError("draw_counts: between 1 and %d groups" % ops.PAIR_DRAWS_MAX_GROUPS)
        eps_e, eps_c = self._draws_noise(dev, n_draws, noise)
        W, _ = self._tail_weights()
        _, counts = ops.pair_probs_draws(lat, eps_e, eps_c, W["pair_classifier.weight"], W["pair_classifier.bias"], self.opt.ec_dim,
                                         labels=labels, groups=groups, n_groups=G, want_prob=False)
        counts = counts.to(torch.int64)
        return (counts, (eps_e, eps_c)) if return_noise else counts

    def get_pair_preds(self, input_ids, att_masks, token_type_ids, round=True):
        """Reference `get_pair_preds` (:265-282): nested python list [[0.|1.], ...]; round=False (newsplit script :442-480): the
        probabilities in the same nesting."""
        prob = self.pair_probabilities(input_ids, att_masks, token_type_ids).reshape(-1, 1).cpu().detach().numpy()
        return (prob.round() if round else prob).tolist()

    # reference helper kept for callers that use it directly (:515-523)
    def get_annealed_weight(self, iteration, lambda_weight):
        return (math.tanh((iteration - self.opt.kl_ann_iterations * 1.5) / (self.opt.kl_ann_iterations / 3)) + 1) * lambda_weight


class FusedAdam:
    """`torch.optim.Adam(model.get_params(), lr)` (ref :936) as ONE HIP kernel over the flat buffer.
    Same defaults and update order; also rewrites the bf16 shadow weights the GEMMs read.  The reference's
    optimiser object is only used through zero_grad()/step() (:840-842), which this class provides.

    fuse_into_backward=True (opt-in): the update of encoder layer l is enqueued on the library's auxiliary stream as
    soon as `loss.backward()` has finished that layer's gradients, so the memory-bound optimiser pass runs beside the
    remaining backward GEMMs; `step()` then only updates what is left (embeddings, pooler, heads) and joins.  Same
    arithmetic, same results -- but the weights move during backward(), so it requires the reference's call pattern
    zero_grad() -> backward() -> step() (no gradient accumulation, no use of the gradients to decide whether to step).
    Under DataParallel (RCCL) each layer's update additionally waits for that layer's gradient all-reduce."""

    def __init__(self, model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, fuse_into_backward=False, param_range=None, params=None):
        """param_range / params (both or neither): a contiguous [lo, hi) slice of the flat buffer and the Parameters in
        it, for models whose get_params() returns several optimiser groups (drl_classifier_en.py:357-376).
        Without them on a model whose get_params() is a tuple (opt.disentangle "vi" / "gan"), the optimiser takes the LAST group, the
        vae-and-classifier one; on a gan model its zero_grad() then clears that group only, like torch -- the same Adam optimiser that
        model.make_fused_optimizers() builds as its third element."""
        model._require_cuda()
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self.step_count = 0
        self._lo, self._hi = (0, model._n_opt) if param_range is None else param_range
        self._clear_all = params is None and not model._gan      # the single-optimiser scripts: zero_grad() clears every .grad of the model
        if params is None:
            gp = model.get_params()              # several groups (vi: 2, gan: 3): the vae group is the last
            params = gp[-1] if isinstance(gp, tuple) else gp
        self._params = list(params)
        self.exp_avg = torch.zeros(self._hi - self._lo, device=model._flat.device, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.grad_scale = 1.0
        self.param_groups = [dict(params=self._params, lr=lr, betas=betas, eps=eps)]
        self._done = []                  # [lo, hi) ranges already updated for the coming step()
        self._skip_count = None
        self._aux = None
        if fuse_into_backward:
            # Two library streams.  Without collectives the updates are queued on the WEIGHT-GRADIENT stream (0), behind the layer's grouped
            # weight-gradient launch that already runs there: measured on one box, alternating (tools/ab_adam_stream.sh, round 4): dense step
            # 7.80-7.85 ms with the update in step(), 7.69-7.72 on the auxiliary stream (1), 7.63-7.71 on the weight-gradient stream;
            # ECPE-shaped 4.38-4.40 / 4.34 / 4.27-4.31.  Under DataParallel an update waits for its bucket's all-reduce, which must not
            # hold up the weight gradients queued behind it: those updates go to the auxiliary stream.
            ptrs = [L.load().carel_side_stream(i) for i in (0, 1)]
            if not all(ptrs):
                raise L.CarelError("carel_side_stream: " + L.load().carel_last_error().decode("utf8", "replace"))
            self._side = torch.cuda.ExternalStream(ptrs[0], device=model._flat.device)
            self._aux = torch.cuda.ExternalStream(ptrs[1], device=model._flat.device)
            self._used = set()
            self._ev = torch.cuda.Event()
            offs, nl = model._offs, model.cfg.layers
            starts = [offs[f"encoder.encoder.layer.{l}.attention.self.query.weight"] for l in range(nl)]
            starts.append(offs["encoder.pooler.dense.weight"])
            self._layer_ranges = [(starts[l], starts[l + 1]) for l in range(nl)]
            model._adam_hook = self

    def zero_grad(self, set_to_none=True):
        for p in (self.model._named.values() if self._clear_all else self._params):
            p.grad = None

    def _adam_args(self, lo, hi):
        """carel_adam_args of the coming step over the flat range [lo, hi): plain Adam, nothing skipped."""
        m = self.model
        a = L.AdamArgs()
        a.param, a.grad = m._flat.data_ptr() + 4 * lo, m._flat_grad.data_ptr() + 4 * lo
        a.exp_avg, a.exp_avg_sq = self.exp_avg.data_ptr() + 4 * (lo - self._lo), self.exp_avg_sq.data_ptr() + 4 * (lo - self._lo)
        a.shadow_bf16 = m._shadow.data_ptr() + 2 * lo
        a.n, a.step = hi - lo, self.step_count + 1
        a.lr, a.beta1, a.beta2, a.eps = self.param_groups[0]["lr"], self.betas[0], self.betas[1], self.eps
        a.grad_scale = self.grad_scale
        a.skip_lo, a.skip_hi, a.skip_flag = 0, 0, None
        return a

    def _launch(self, lo, hi, stream, with_skip):
        m = self.model
        a = self._adam_args(lo, hi)
        call = getattr(m, "_last_call", None)
        if with_skip and m._has_pair_skip and call is not None and lo <= m._pair_lo and m._pair_hi <= hi:
            # the pair head keeps its weights/moments when its loss term was replaced by 0
            a.skip_lo, a.skip_hi = m._pair_lo - lo, m._pair_hi - lo
            off = L.load().carel_tail_pair_dead_offset(call.B, m.opt.ec_dim, m.opt.pair_bow_dim)
            a.skip_flag = call.buf.work.data_ptr() + off * 4
            if self._skip_count is None:       # frozen steps of the pair head so far (torch: that parameter's own step counter lags)
                self._skip_count = torch.zeros(1, device=m._flat.device, dtype=torch.float32)
            a.skip_count = self._skip_count.data_ptr()
        L.check(L.load().carel_adam_step(C.byref(a), stream), "carel_adam_step")

    def _layer_ready(self, layer, after=None):
        """Called by the model's backward when encoder layer `layer` has all its gradients on the main stream; under
        DataParallel `after` is the work handle of the layer's gradient all-reduce (RCCL), which the update waits for."""
        self._range_ready(self._layer_ranges[layer], after)

    def _range_ready(self, rng, after=None):
        """Update the flat range [lo, hi) on the auxiliary stream, after the main stream's work so far (`after` None) or after the
        collective behind the handle `after` (its wait() orders the auxiliary stream only)."""
        lo, hi = rng
        if after is not None:
            st = self._aux
            with torch.cuda.stream(st):
                after.wait()                 # stream-side wait: the auxiliary stream blocks until the collective is done
        else:
            st = self._aux if os.environ.get("CAREL_ADAM_STREAM") == "1" else self._side      # (the variable: A/B tool only, tools/ab_adam_stream.sh)
            self._ev.record()
            st.wait_event(self._ev)
        self._used.add(st)
        self._launch(lo, hi, C.c_void_p(st.cuda_stream), with_skip=False)
        self._done.append((lo, hi))

    def _join(self):
        if self._aux is not None and self._done:
            for st in self._used:
                torch.cuda.current_stream().wait_stream(st)
            self._used.clear()

    def step(self):
        m = self.model
        lo = self._lo
        for dlo, dhi in sorted(self._done):             # whatever backward() has not updated yet
            if dlo > lo:
                self._launch(lo, dlo, L.current_stream(), with_skip=True)
            lo = max(lo, dhi)
        if lo < self._hi:
            self._launch(lo, self._hi, L.current_stream(), with_skip=True)
        self._join()
        self._done = []
        self.step_count += 1
        m.mark_shadow_fresh()

    def state_dict(self):
        return dict(step=self.step_count, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr,
                    pair_head_frozen_steps=None if self._skip_count is None else self._skip_count.clone())

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        fr = sd.get("pair_head_frozen_steps")
        self._skip_count = None if fr is None else fr.to(self.exp_avg.device, torch.float32).reshape(1).clone()


class FusedRMSprop:
    """`torch.optim.RMSprop(params, lr)` (torch defaults) over one contiguous range of the model's flat buffer; used through
    zero_grad() / step() like the discriminator optimisers of drl_classifier_en.py (:919-947, :1056-1060) and drl_classifier_ec_gan.py (:784-802, :903-908)."""

    def __init__(self, model, lr, param_range, params, alpha=0.99, eps=1e-8):
        model._require_cuda()
        self.model, self.lr, self.alpha, self.eps = model, lr, alpha, eps
        self._lo, self._hi = param_range
        self._params = list(params)
        self.square_avg = torch.zeros(self._hi - self._lo, device=model._flat.device, dtype=torch.float32)
        self.param_groups = [dict(params=self._params, lr=lr, alpha=alpha, eps=eps)]

    def zero_grad(self, set_to_none=True):
        for p in self._params:
            p.grad = None

    def step(self):
        m = self.model
        if any(p.grad is None for p in self._params):
            return                                   # torch skips parameters without a gradient
        L.check(L.load().carel_rmsprop_step(m._flat.data_ptr() + 4 * self._lo, m._flat_grad.data_ptr() + 4 * self._lo, self.square_avg.data_ptr(),
                                            self._hi - self._lo, self.param_groups[0]["lr"], self.alpha, self.eps, L.current_stream()),
                "carel_rmsprop_step")

    def state_dict(self):
        return dict(square_avg=self.square_avg, lr=self.lr)

    def load_state_dict(self, sd):
        self.square_avg.copy_(sd["square_avg"])
