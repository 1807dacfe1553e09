"""Inputs, the oracle side and the HIP side of the VAE-tail tests (tests/test_gpu_tail.py, tests/test_gpu_tail_sweep.py): the pooler
and everything after it (oracle.carel_oracle.tail_forward, imported and not edited) at any latent width / emotion head / dtype, and
one run of carel_tail_latents -> carel_tail_losses -> carel_tail_backward through carel_vae_amd.ops with every output pre-filled
with NaN.  The oracle works in float32 (autograd on the CPU: the yardstick of test_gpu_tail.py) and in float64 on the same float32
inputs (dtype=torch.float64: the yardstick of the sweep)."""
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from oracle import carel_oracle as O
from tests.gpu_util import Guarded

TAIL_KEYS = ["encoder.pooler.dense.weight", "encoder.pooler.dense.bias",
             "emotion_mu.weight", "emotion_mu.bias", "emotion_log_var.weight", "emotion_log_var.bias",
             "cause_mu.weight", "cause_mu.bias", "cause_log_var.weight", "cause_log_var.bias",
             "emotion_classifier.weight", "emotion_classifier.bias", "cause_classifier.weight", "cause_classifier.bias",
             "pair_classifier.weight", "pair_classifier.bias", "decoder.weight", "decoder.bias"]
# what carel_tail_backward scales by grad_out (d lat and everything behind it); the classifier and decoder gradients of
# carel_tail_losses are left to the caller (include/carel_hip.h)
SCALED_BY_GRAD_OUT = TAIL_KEYS[:10]


def setup(B, S, V, seed, all_negative=False, ec_dim=24, e_num_class=6, disentangle="mmd", emotion_head="ce"):
    """Weights, the encoder's last hidden state [B*S, 768], labels and the two noise vectors.  Emotion labels are taken modulo
    e_num_class (CE head) or binarised (one-logit BCE head, as test_hsic_variant_of_the_tail does)."""
    cfg = O.EncoderConfig(layers=0, vocab_size=50)
    opt = O.Opt(pair_bow_dim=V, ec_dim=ec_dim, e_num_class=e_num_class)
    opt.disentangle, opt.emotion_head = disentangle, emotion_head
    P = {k: v for k, v in O.init_params(cfg, opt, seed=seed).items() if k in TAIL_KEYS}
    g = torch.Generator().manual_seed(seed)
    P["encoder.pooler.dense.weight"] = torch.randn((768, 768), generator=g) * 0.05
    x_last = torch.randn((B * S, 768), generator=g)
    batch = O.synthetic_batch(B, 8, O.EncoderConfig(layers=1, vocab_size=50), V, seed=seed)
    if emotion_head == "bce":
        batch["emo_labels"] = (batch["emo_labels"] > 2).to(torch.int64)
    else:
        batch["emo_labels"] = batch["emo_labels"] % e_num_class
    if all_negative:
        batch["labels"].zero_(); batch["cau_labels"].zero_()
    eps_e, eps_c = torch.randn(ec_dim, generator=g), torch.randn(ec_dim, generator=g)
    return cfg, opt, P, x_last, batch, eps_e, eps_c


def oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, it, train, seed, dtype=None, dz=None, grad_out=None, **kw):
    """-> (tail_forward's dict, pooled, {key: gradient or None}, d x_last).  dtype: the arithmetic of the oracle (weights, x_last and
    the noise are cast to it; labels and dropout masks are exact in either).  dz [B, 2 * ec_dim] / grad_out (float): the gradients are
    those of grad_out * loss + sum([z_e | z_c] * dz) -- an extra gradient on the sampled embeddings, which grad_out does not scale
    (ops.tail_backward's dz_extra); without either, of the loss."""
    cast = (lambda t: t.clone()) if dtype is None else (lambda t: t.to(dtype))
    Pg = {k: cast(v).requires_grad_(True) for k, v in P.items()}
    xg = cast(x_last).requires_grad_(True)
    kw.setdefault("disentangle", getattr(opt, "disentangle", "mmd"))
    kw.setdefault("emotion_head", getattr(opt, "emotion_head", "ce"))
    pooled = torch.tanh(xg.view(B, S, 768)[:, 0] @ Pg["encoder.pooler.dense.weight"].t() + Pg["encoder.pooler.dense.bias"])
    out = O.tail_forward(Pg, pooled, batch["emo_labels"], batch["cau_labels"], batch["labels"], batch["bow_reps"], it, opt,
                         cast(eps_e), cast(eps_c), train=train, seed=seed, **kw)
    if dz is None and grad_out is None:
        out["loss"].backward()
    else:
        obj = out["loss"] * (1.0 if grad_out is None else grad_out)
        if dz is not None:
            obj = obj + (torch.cat((out["z_e"], out["z_c"]), dim=1) * cast(dz)).sum()
        obj.backward()
    return out, pooled, {k: v.grad for k, v in Pg.items()}, xg.grad


def hip_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, V, it, drop, serial=0, grad_out=None, guard=None, dz_extra=None, **kw):
    """One latents -> losses -> backward run; every output (and the workspace) starts as NaN.  grad_out: float, passed to
    carel_tail_backward as a device scalar.  dz_extra: f32 [B, 2 * ec_dim] (any device), the extra gradient on the sampled embeddings
    of carel_tail_backward_dz.  guard: a torch.Generator -> the workspace (at exactly carel_tail_workspace_floats),
    dx_last, z and the decoder gradients sit in tests.gpu_util.Guarded allocations, listed in buf.guards."""
    dev, nan, D = "cuda", float("nan"), opt.ec_dim
    W = {k: v.to(dev) for k, v in P.items()}
    G = {k: torch.full_like(v, nan) for k, v in W.items()}
    buf = ops.TailBuffers(B, S, D, opt.e_num_class, V, dev)
    buf.guards = []
    if guard is not None:
        gd = dict(work=Guarded((L.load().carel_tail_workspace_floats(B, D, V),), torch.float32, nan, guard),
                  dx_last=Guarded((B * S, 768), torch.float32, nan, guard), z=Guarded((B, 2 * D), torch.float32, nan, guard))
        buf.work, buf.dx_last, buf.z = gd["work"].t, gd["dx_last"].t, gd["z"].t
        for k in ("decoder.weight", "decoder.bias"):
            gd[k] = Guarded(tuple(W[k].shape), torch.float32, nan, guard)
            G[k] = gd[k].t
        buf.guards = list(gd.items())
    for t in (buf.pooled, buf.lat, buf.z, buf.terms[:9], buf.work, buf.dx_last):      # (terms[9:] are not the tail's)
        t.fill_(nan)
    labels = dict(emo=batch["emo_labels"].to(dev).view(-1).contiguous(), cau=batch["cau_labels"].to(dev).view(-1).contiguous(),
                  pair=batch["labels"].to(dev).view(-1).contiguous(), bow=batch["bow_reps"].to(dev).contiguous())
    xl, ee, ec = x_last.to(dev), eps_e.to(dev), eps_c.to(dev)
    a = ops.tail_args(buf, xl, W, labels, ee, ec, opt, ops.kl_anneal_weight(it, opt), grads=G, drop=drop, **kw)
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=dev)
    dz = None if dz_extra is None else dz_extra.to(dev, torch.float32).contiguous()
    a._keep = (W, G, labels, xl, ee, ec, go, dz)  # tail_args holds addresses only: the noise must outlive the calls, or go takes its block
    a.serial = serial
    ops.tail_latents(a)
    ops.tail_losses(a)
    ops.tail_backward(a, go, dz)
    torch.cuda.synchronize()
    return buf, G
