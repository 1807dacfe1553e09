"""The float64 yardstick of the three-space tail (csrc/en_tail.hip and its use of rowvec_device.h), the case builders of its sweep,
the limits restated from its host code and the ctypes driver of the two losses entry points.  Used by
tests/test_en_tail_restate_host.py (CPU) and tests/test_gpu_en_tail_sweep.py / tests/test_gpu_en_bow_kernels.py (GPU).

The arithmetic is tests/en_bow_restate.tail_from_latents (imported, not restated): `reference` runs it in the dtype asked for and takes
every output of carel_en_tail_losses / carel_en_tail_losses_bow from it by autograd -- the 21 terms, z, and per parameter the images of
DESIGN.md "Config 4": `own` (gradient of the discriminator's own loss: g_cdisc_*[0], g_sdisc_*), `second` (content_disc's loss on the
cause sample: g_cdisc_*[1]) and `entropy-share` (gradient of the vae loss, which reaches a discriminator only through its entropy term
and therefore carries w_con_adv / w_ec_adv / w_ecce_adv: g_cdisc_*[2], g_sdisc_ent_*); classifier / decoder gradients and d lat are
gradients of the vae loss.  `front` / `back` are the pooler and the six latent heads around it.

BOUNDS.  Every comparison is per element, |got - ref| <= bound, bound = c * 2^-24 * scale:
  images and vectors                scale = max|ref| of the tensor
  dlat, dx_last, pooled, lat, z     scale = max|ref| of the row
  scalars (the 21 terms, and the one-logit bias gradients, which are one number each)
                                    scale = sum of |addend| over the samples in the float64 restatement.  Every term but the total is a
                                    mean of same-signed addends (BCE >= 0, p log p <= 0, KL elements >= 0), so its scale is |term|;
                                    the total's is sum_i |w_i| |term_i| (the entropies are negative); a one-logit bias gradient is
                                    sum_b dloss/dlogit_b with both signs: scale = sum_b |dloss/dlogit_b| (taken by autograd from a
                                    per-sample copy of the bias).
  g_cdisc_w[2] / g_cdisc_b[2]       scale PER ELEMENT = the sum of the addends' magnitudes, see below.
c is chosen per quantity on the CPU (tests/test_en_tail_restate_host.py::test_float32_torch_stays_within_half_of_every_bound): the
smallest power of two for which THE SAME restatement in float32 (stock torch; the reference alone, never the kernel) stays within half
the bound on every case of the sweep.  The kernels get that bound times 4 (KERNEL_MARGIN): __expf / __logf / __frcp_rn at ~1 ulp each,
the seven-term series of log(1 - p), and a different, fixed summation tree.

THE ENTROPY IMAGES.  DESIGN.md section 7 shows g_cdisc_w[2] / g_cdisc_b[2] at 7.4e-6 / 1.2e-5 relative norm where everything else is at
<= 7e-7.  That is the arithmetic, not a defect: with a_j = log(p_j + eps) + p_j / (p_j + eps),
    d/dlogit_j  sum_k p_k log(p_k + eps)  =  p_j (a_j - sum_k p_k a_k)  =  p_j (a_j - de),
and on a softmax over V words that is close to uniform, a_j and de are both about 1 - log V (-4.3 at V = 211, -8.7 at V = 23 771) while
their difference is the logit's deviation from the row's mean, a few tenths for these inputs: the subtraction loses log V / |a_j - de|, a
factor 10-50, whichever way it is evaluated (float32 torch's softmax backward loses the same).  The image element
sum_b x_bk p_bj (a_bj - de_b) s_ent therefore has rounding error proportional to sum_b |x_bk| p_bj (|a_bj| + |de_b|) s_ent, and that is
its scale (`entropy_scale`), per element.  Measured: on the scale of max|ref| float32 torch itself
sits at 64 (w) and 27 (b) units of 2^-24 on this sweep where the other vocabulary-wide images sit at 6-22, i.e. it would need c = 128 / 64;
on the addend scale it needs 64 / 32 like content_disc's other images.  The kernel stays within 0.063 / 0.094 of its bound on the addend
scale (0.20 / 0.39 of 4 * 64 / 4 * 32 on the scale of max|ref|, i.e. 51 / 50 units against float32 torch's 64 / 27: the same
order), so the larger relative norm in that table is this cancellation and nothing else.  No kernel change.

The chosen c, the float32-torch fraction of the bound (CPU) and the worst kernel fraction over the GPU sweep (MI355X) per quantity:
see C_BOUND below and the table in DESIGN.md section 7.
"""
import re
from functools import lru_cache
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from tests import en_bow_restate as R

TH = 768
SMALL = ("emotion_disc", "cause_disc", "ec_disc", "ce_disc")                     # sdisc_w[0..3]; own losses T[2], T[4], T[3], T[5]
ONE_LOGIT = SMALL + ("emotion_classifier", "cause_classifier", "pair_classifier")
TERM_NAMES = ("content_disc_emo", "content_disc_cau", "emotion_disc", "ec_disc", "cause_disc", "ce_disc", "vae", "cent_e", "cent_c", "ent_ed",
              "ent_cad", "ent_ec", "ent_ce", "emo_mul", "cau_mul", "con_mul", "pair", "kl_e", "kl_c", "kl_con", "rec")
PAIR_DEPENDENT = ("terms", "d_pair_w", "d_pair_b", "dlat")       # what the pos_weight override may move (of the terms: 6 and 16)
KERNEL_MARGIN = 4.0
U = 2.0 ** -24


def head_shapes(V, Cd, D):
    return dict(content_disc=(V, D), content_classifier=(V, Cd), decoder=(V, 2 * D + Cd), emotion_disc=(1, Cd), cause_disc=(1, Cd),
                ec_disc=(1, D), ce_disc=(1, D), emotion_classifier=(1, D), cause_classifier=(1, D), pair_classifier=(1, 2 * D))


def image_shapes(B, V, Cd, D):
    """Every image of the losses call, in the order the driver allocates them."""
    s = {}
    for i in range(3):
        s["g_cdisc_w%d" % i], s["g_cdisc_b%d" % i] = (V, D), (V,)
    for i, h in enumerate(SMALL):
        k = head_shapes(V, Cd, D)[h]
        s["g_sdisc_w%d" % i], s["g_sdisc_b%d" % i], s["g_sdisc_ent_w%d" % i], s["g_sdisc_ent_b%d" % i] = k, (1,), k, (1,)
    s.update(d_ccls_w=(V, Cd), d_ccls_b=(V,), d_emo_w=(1, D), d_emo_b=(1,), d_cau_w=(1, D), d_cau_b=(1,), d_pair_w=(1, 2 * D), d_pair_b=(1,),
             d_dec_w=(V, 2 * D + Cd), d_dec_b=(V,))
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# limits restated from the host code of csrc/en_tail.hip
# ---------------------------------------------------------------------------------------------------------------------------
def al(n):
    return (n + 63) & ~63


def en_splits(V):
    return max(1, min(64, (V + 255) // 256))


def split_plan(K, splits=None):
    """sgemm()'s split of a reduction of length K: (splits asked for, kchunk, non-empty chunks nz).  The tail asks for en_splits(V) =
    min(64, ceil(V / 256)); nz < splits is the branch that clears the empty slabs."""
    if splits is None:
        splits = en_splits(K)
    kchunk = ((K + splits - 1) // splits + 31) & ~31
    return splits, kchunk, (K + kchunk - 1) // kchunk


def heads_lds_bytes(B):
    """Dynamic LDS of en_heads_kernel: red[16], lg[7][B], dl[7][B], de[4][B]; above 64 KB the host sets the function attribute first."""
    return 4 * (16 + 18 * B)


def carve(B, D, Cd, V):
    """en_carve: name -> offset in floats, and "total"."""
    ZW, LW = 2 * D + Cd, 2 * Cd + 4 * D
    o, w = 0, {}
    seg_k = (D, D, Cd, Cd, D, D, Cd, D, D, 2 * D)             # the ten dropped-out copies, sites 110..119
    w["xd"] = [0] * 10
    for s, k in enumerate(seg_k):
        w["xd"][s] = o
        o += al(B * k)
    hc, pc = (2 * Cd + 31) // 32 + (4 * D + 31) // 32, TH // 32
    chunks = (V + 2047) // 2048
    for name, n in (("L1", B * V), ("L2", B * V), ("rowstat", 8 * B), ("dxd_cmul", B * Cd), ("dz_dec", B * ZW), ("dz_heads", B * 2 * D),
                    ("parts", en_splits(V) * B * ZW), ("dlat", B * LW), ("dpooled", B * TH), ("dpre", B * TH), ("dcls", B * TH),
                    ("dgpart", max(hc, pc) * B * TH), ("rowpart", B * chunks * 2), ("rowpart2", B * chunks * 4), ("lg", 7 * B), ("klrow", 3 * B)):
        w[name] = o
        o += al(n)
    w["total"] = o
    w["seg_k"] = seg_k
    return w


def work_offsets(B, Cd, V, D=24):
    """The hand-written closed form the kernel test has used for rowstat and dlat (checked against `carve` on the CPU)."""
    ZW = 2 * D + Cd
    o = sum(al(B * k) for k in (D, D, Cd, Cd, D, D, Cd, D, D, 2 * D)) + 2 * al(B * V)
    rowstat = o
    o += al(8 * B) + al(B * Cd) + al(B * ZW) + al(B * 2 * D) + al(min(64, (V + 255) // 256) * B * ZW)
    return rowstat, o


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Spec(NamedTuple):
    B: int
    V: int
    Cd: int
    D: int = 24
    p: float = 0.0
    peaked: bool = False
    off: int = 0             # drop_row_offset

    @property
    def id(self):
        return "B%d-V%d-Cd%d-D%d" % self[:4] + ("-p%g" % self.p if self.p else "") + ("-peaked" if self.peaked else "") + ("-off%d" % self.off if self.off else "")


PEAK_CDISC, PEAK_DEC = 3, 5


def peaked(c):
    """One content-discriminator and one decoder logit a fixed gap above the rest: the other logits are within a few tenths of 0, so
    with gap = log V + 4.5 the peak has p ~ 1 / (1 + exp(-4.5)) = 0.989.  1 - p >= 1e-3 (asserted): the softmax is peaked, not saturated."""
    gap = float(torch.log(torch.tensor(float(c.V)))) + 4.5
    c.P["content_disc.bias"][PEAK_CDISC] += gap
    c.P["decoder.bias"][PEAK_DEC] += gap
    D, f = c.D, torch.float64
    z = latents_to_z(c.lat.to(f), c.eps.to(f), D, c.Cd)
    for x, head in ((z[:, :D], "content_disc"), (z[:, D:2 * D], "content_disc"), (z, "decoder")):
        pmax = torch.softmax(x @ c.P[head + ".weight"].to(f).t() + c.P[head + ".bias"].to(f), dim=1).max(dim=1).values
        assert float(pmax.min()) > 0.9 and float((1 - pmax).min()) >= 1e-3, (head, float(pmax.min()), float(pmax.max()))


def latents_to_z(lat, eps, D, Cd):
    """z = [emotion | cause | content] samples from the kernel's lat layout; eps = [e | c | con]."""
    mu_con, lv_con, mu_e, lv_e, mu_c, lv_c = (lat[:, a:b] for a, b in zip((0, Cd, 2 * Cd, 2 * Cd + D, 2 * Cd + 2 * D, 2 * Cd + 3 * D),
                                                                          (Cd, 2 * Cd, 2 * Cd + D, 2 * Cd + 2 * D, 2 * Cd + 3 * D, 2 * Cd + 4 * D)))
    return torch.cat((mu_e + eps[:D] * lv_e.exp(), mu_c + eps[D:2 * D] * lv_c.exp(), mu_con + eps[2 * D:] * lv_con.exp()), dim=1)


def make_case(B, V, Cd, D=24, seed=0, drop_p=0.0, edit=None, off=0):
    """Seeded inputs of one losses call: weights uniform in +-1/sqrt(K), latents 0.3 randn, a 5 % dense bag of words, pair[0] = 1 and
    pair[1] = 0 (pos_weight = (B - sum y) / sum y is finite, and non-zero from B = 2)."""
    g = torch.Generator().manual_seed(seed)
    opt = OE.OptEn(pair_bow_dim=V, con_dim=Cd, ec_dim=D, dropout=drop_p)
    P = {}
    for name, s in head_shapes(V, Cd, D).items():
        bound = 1.0 / s[1] ** 0.5
        P[name + ".weight"] = (torch.rand(s, generator=g) * 2 - 1) * bound
        P[name + ".bias"] = (torch.rand(s[0], generator=g) * 2 - 1) * bound
    lat = torch.randn(B, 2 * Cd + 4 * D, generator=g) * 0.3
    eps = torch.randn(2 * D + Cd, generator=g)
    bow = (torch.rand(B, V, generator=g) < 0.05).float()
    emo, cau = (torch.rand(B, generator=g) < 0.5).float(), (torch.rand(B, generator=g) < 0.5).float()
    pair = (torch.rand(B, generator=g) < 0.4).float()
    pair[0] = 1.0
    if B > 1:
        pair[1] = 0.0
    c = SimpleNamespace(B=B, V=V, Cd=Cd, D=D, opt=opt, P=P, lat=lat, eps=eps, bow=bow, emo=emo, cau=cau, pair=pair, drop_p=drop_p,
                        seed=1234 + seed, kl=(0.013, 0.021), off=off)
    if edit is not None:
        edit(c)
    return c


@lru_cache(maxsize=None)
def _case_of(spec: Spec):
    return make_case(spec.B, spec.V, spec.Cd, spec.D, seed=spec.B * 7 + spec.V + spec.Cd + 3 * spec.D, drop_p=spec.p,
                     edit=peaked if spec.peaked else None, off=spec.off)


def copy_case(c):
    """A case whose tensors are the caller's own: editing it cannot reach another test."""
    s = SimpleNamespace(**vars(c))
    s.P = {k: v.clone() for k, v in c.P.items()}
    for k in ("lat", "eps", "bow", "emo", "cau", "pair"):
        setattr(s, k, getattr(c, k).clone())
    return s


def case_of(spec: Spec):
    return copy_case(_case_of(spec))


def shard(c, lo, hi, off=None):
    """Rows lo..hi of a case as a case of its own at drop_row_offset c.off + lo (or `off`): what one data-parallel rank sees."""
    s = SimpleNamespace(**vars(c))
    s.B, s.off = hi - lo, c.off + lo if off is None else off
    for k in ("lat", "bow", "emo", "cau", "pair"):
        setattr(s, k, getattr(c, k)[lo:hi].clone())
    return s


BATCH_EDGES = [Spec(B, 70, 4) for B in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 909, 910, 1024)] + [Spec(1024, 70, 384)]
WIDTH_EDGES = [Spec(B, 211, Cd, D) for D in (2, 24, 62, 64) for Cd in (4, 128, 508, 1024) for B in (5, 13)]
VOCAB_EDGES = [Spec(5, V, 4) for V in (2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)] + [Spec(5, 2049, 384), Spec(2, 16385, 4)]
PEAKED = [Spec(5, 2049, 384, peaked=True)]
DROPOUT = [Spec(B, V, Cd, p=0.5, off=off) for (B, V, Cd) in ((16, 211, 384), (65, 2049, 4)) for off in (0, 8)]
PLAIN_CASES = BATCH_EDGES + WIDTH_EDGES + VOCAB_EDGES + PEAKED + DROPOUT
BOW_CASES = [Spec(1, 70, 4), Spec(65, 2049, 384), Spec(910, 70, 4), Spec(5, 16385, 4), Spec(16, 211, 384, p=0.5)]
ALL_CASES = [(s, "plain") for s in PLAIN_CASES] + [(s, "bow") for s in BOW_CASES]
assert len(set(ALL_CASES)) == len(ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: every output of the losses call, and the scale of each
# ---------------------------------------------------------------------------------------------------------------------------
def entropy_scale(c, P, z, dt, off):
    """sum_b |x_bk| p_bj (|a_bj| + |de_b|) w_con_adv / B over both content-discriminator calls (module docstring)."""
    D, o = c.D, c.opt
    W, b = P["content_disc.weight"].detach(), P["content_disc.bias"].detach()
    sw, sb = torch.zeros_like(W), torch.zeros_like(b)
    for x, site in ((z[:, :D], OE.SITE_CDISC_E), (z[:, D:2 * D], OE.SITE_CDISC_C)):
        m = O.dropout_scale_mask(c.seed, site, tuple(x.shape), c.drop_p, off)
        x = x if m is None else x * m.to(dt)
        p = torch.softmax(x @ W.t() + b, dim=1)
        a = torch.log(p + o.epsilon) + p / (p + o.epsilon)
        mag = p * (a.abs() + (p * a).sum(dim=1, keepdim=True).abs())
        sw += mag.t() @ x.abs()
        sb += mag.sum(dim=0)
    return sw * (o.con_adv_loss_weight / c.B), sb * (o.con_adv_loss_weight / c.B)


def reference(c, weighting="plain", dtype=torch.float64, pos_weight=None):
    """-> (ref, scale): name -> tensor for the 21 `terms`, `z`, every image and `dlat`; scale as the module docstring defines it
    (a float, a [B, 1] column for the per-row quantities, a tensor for the per-element ones)."""
    dt, B, D, o = dtype, c.B, c.D, c.opt
    P = {k: v.to(dt) for k, v in c.P.items()}
    for h in ONE_LOGIT:          # a per-sample copy of the bias: same values, and its gradient is dloss / dlogit_b
        P[h + ".bias"] = P[h + ".bias"].reshape(1, 1).repeat(B, 1)
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    lat = c.lat.to(dt).requires_grad_(True)
    eps = dict(e=c.eps[:D].to(dt), c=c.eps[D:2 * D].to(dt), con=c.eps[2 * D:].to(dt))
    out = R.tail_from_latents(P, R.split_lat(lat, o), c.emo, c.cau, c.pair, c.bow.to(dt), c.kl[0], c.kl[1], o, eps, weighting=weighting,
                              train=c.drop_p > 0, seed=c.seed, row_offset=c.off, pos_weight=pos_weight)
    ref, scale = {}, {}
    t = torch.stack([out[n].detach() for n in TERM_NAMES])
    ts = t.abs()
    wt = dict(cent_e=o.con_adv_loss_weight, cent_c=o.con_adv_loss_weight, ent_ed=o.ec_adv_loss_weight, ent_cad=o.ec_adv_loss_weight,
              ent_ec=o.ecce_adv_loss_weight, ent_ce=o.ecce_adv_loss_weight, emo_mul=o.ec_mul_loss_weight, cau_mul=o.ec_mul_loss_weight,
              con_mul=o.con_mul_loss_weight, pair=o.pair_mul_loss_weight, kl_e=1.0, kl_c=1.0, kl_con=1.0, rec=1.0)
    ts[6] = sum(w * ts[TERM_NAMES.index(n)] for n, w in wt.items())
    ref["terms"], scale["terms"] = t, ts
    ref["z"] = out["z"].detach()

    def grads(loss, heads):
        keys = [h + s for h in heads for s in (".weight", ".bias")]
        g = torch.autograd.grad(loss, [P[k] for k in keys], retain_graph=True)
        return dict(zip(keys, g))

    def put(name, g):          # a one-logit bias gradient arrives per sample
        if g.dim() == 2 and re.search(r"_b\d?$", name):          # (a vocabulary-wide head's bias gradient is one-dimensional)
            ref[name], scale[name] = g.sum().reshape(1), float(g.abs().sum())
        else:
            ref[name], scale[name] = g, float(g.abs().max())
    g = grads(out["content_disc_emo"], ["content_disc"])
    put("g_cdisc_w0", g["content_disc.weight"]), put("g_cdisc_b0", g["content_disc.bias"])
    g = grads(out["content_disc_cau"], ["content_disc"])
    put("g_cdisc_w1", g["content_disc.weight"]), put("g_cdisc_b1", g["content_disc.bias"])
    for i, h in enumerate(SMALL):
        g = grads(out[h], [h])
        put("g_sdisc_w%d" % i, g[h + ".weight"]), put("g_sdisc_b%d" % i, g[h + ".bias"])
    heads = ["content_disc", "content_classifier", "decoder", "emotion_classifier", "cause_classifier", "pair_classifier"] + list(SMALL)
    keys = [h + s for h in heads for s in (".weight", ".bias")]
    gv = torch.autograd.grad(out["vae"], [P[k] for k in keys] + [lat])
    g = dict(zip(keys, gv[:-1]))
    put("g_cdisc_w2", g["content_disc.weight"]), put("g_cdisc_b2", g["content_disc.bias"])
    with torch.no_grad():
        scale["g_cdisc_w2"], scale["g_cdisc_b2"] = entropy_scale(c, P, ref["z"], dt, c.off)
    for i, h in enumerate(SMALL):
        put("g_sdisc_ent_w%d" % i, g[h + ".weight"]), put("g_sdisc_ent_b%d" % i, g[h + ".bias"])
    for n, h in (("d_ccls", "content_classifier"), ("d_emo", "emotion_classifier"), ("d_cau", "cause_classifier"), ("d_pair", "pair_classifier"),
                 ("d_dec", "decoder")):
        put(n + "_w", g[h + ".weight"]), put(n + "_b", g[h + ".bias"])
    ref["dlat"] = gv[-1]
    for k in ("z", "dlat"):
        scale[k] = ref[k].abs().max(dim=1, keepdim=True).values
    ref["pos_weight"] = (B - c.pair.sum()) / c.pair.sum() if pos_weight is None else torch.as_tensor(pos_weight)
    return ref, scale


@lru_cache(maxsize=None)
def reference_of(spec: Spec, weighting: str):
    """The float64 reference of a case of the sweep, computed once for every test that needs it (and not to be edited)."""
    return reference(_case_of(spec), weighting)


def make_front(B, Cd, D, seq_len, irregular, seed):
    """Inputs of carel_en_tail_latents / carel_en_tail_backward: the last encoder output [n_rows, 768] with the [CLS] rows either
    dense (row b * seq_len) or given by an irregular, increasing `cls_rows` with n_rows past the last one; pooler and the six heads."""
    g = torch.Generator().manual_seed(seed)
    LW = 2 * Cd + 4 * D
    if irregular:
        rows = torch.cumsum(torch.randint(1, 4, (B,), generator=g), 0)          # the first [CLS] row is not row 0 either
        n_rows = int(rows[-1]) + 3
    else:
        rows, n_rows = torch.arange(B) * seq_len, B * seq_len
    u = lambda *s: (torch.rand(s, generator=g) * 2 - 1) / TH ** 0.5      # noqa: E731
    widths = (Cd, Cd, D, D, D, D)
    return SimpleNamespace(B=B, Cd=Cd, D=D, seq_len=seq_len, rows=rows.to(torch.int32), n_rows=n_rows, irregular=irregular,
                           x_last=torch.randn(n_rows, TH, generator=g), pooler_w=u(TH, TH), pooler_b=u(TH), head_w=[u(n, TH) for n in widths],
                           head_b=[u(n) for n in widths], dlat=torch.randn(B, LW, generator=g) * 0.01)


def front(f, dtype=torch.float64, x_cls=None, P=None):
    """pooled = tanh(x_cls Wp^T + bp) and the six latent heads in the kernel's lat layout [mu_con | lv_con | mu_e | lv_e | mu_c | lv_c]."""
    x = f.x_last.to(dtype)[f.rows.long()] if x_cls is None else x_cls
    Wp, bp = (f.pooler_w.to(dtype), f.pooler_b.to(dtype)) if P is None else P
    pooled = torch.tanh(x @ Wp.t() + bp)
    lat = torch.cat([pooled @ w.to(dtype).t() + b.to(dtype) for w, b in zip(f.head_w, f.head_b)], dim=1)
    return pooled, lat


def back(f, grad_out=None, dtype=torch.float64):
    """Given g * dlat: d_pooler_w, d_pooler_b and dx_last [n_rows, 768], exactly zero on every row that is not a [CLS] row."""
    x = f.x_last.to(dtype)[f.rows.long()].requires_grad_(True)
    Wp, bp = f.pooler_w.to(dtype).requires_grad_(True), f.pooler_b.to(dtype).requires_grad_(True)
    _, lat = front(f, dtype, x, (Wp, bp))
    up = f.dlat.to(dtype) * (1.0 if grad_out is None else torch.tensor(grad_out, dtype=torch.float32).to(dtype))
    dW, db, dx = torch.autograd.grad((lat * up).sum(), [Wp, bp, x])
    dx_last = torch.zeros(f.n_rows, TH, dtype=dtype)
    dx_last[f.rows.long()] = dx
    return dict(d_pooler_w=dW, d_pooler_b=db, dx_last=dx_last)


# ---------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------
def family(name):
    """The quantity a constant belongs to: the four one-logit discriminators share theirs, content_disc's own and second image too."""
    if name in ("g_cdisc_w2", "g_cdisc_b2"):
        return "g_cdisc_ent_" + name[8]
    return re.sub(r"\d$", "", name)


# quantity: c.  Beside each: float32 torch's worst |err| / (2^-24 scale) over ALL_CASES on the CPU (so c >= twice that), and the worst
# fraction of the kernel's bound (4 c 2^-24 scale) over tests/test_gpu_en_tail_sweep.py on an MI355X.
C_BOUND = {
    # quantity: c                  float32 torch (CPU)   kernel, fraction of 4 c (MI355X)
    "term_content_disc_emo": 8,    # 2.66                0.089
    "term_content_disc_cau": 8,    # 2.67                0.112
    "term_emotion_disc": 8,        # 2.62                0.094
    "term_ec_disc": 8,             # 2.51                0.103
    "term_cause_disc": 8,          # 2.77                0.088
    "term_ce_disc": 8,             # 2.72                0.099
    "term_vae": 8,                 # 2.33                0.083
    "term_cent_e": 64,             # 21.84 (peaked)      0.144
    "term_cent_c": 128,            # 39.59 (peaked)      0.020
    "term_ent_ed": 8,              # 2.86                0.105
    "term_ent_cad": 8,             # 3.74                0.105
    "term_ent_ec": 8,              # 2.82                0.117
    "term_ent_ce": 8,              # 2.77                0.110
    "term_emo_mul": 8,             # 2.91                0.109
    "term_cau_mul": 8,             # 3.40                0.092
    "term_con_mul": 8,             # 3.41                0.116
    "term_pair": 8,                # 2.76                0.067
    "term_kl_e": 8,                # 3.14                0.130
    "term_kl_c": 8,                # 2.93                0.130
    "term_kl_con": 16,             # 4.01                0.077
    "term_rec": 8,                 # 2.47                0.101
    "z": 8,                        # 2.48                0.057
    "g_cdisc_w": 64,               # 21.99 (peaked)      0.171
    "g_cdisc_b": 64,               # 21.94 (peaked)      0.130
    "g_cdisc_ent_w": 64,           # 16.32 (peaked)      0.063
    "g_cdisc_ent_b": 32,           # 11.22 (peaked)      0.094
    "g_sdisc_w": 32,               # 14.37               0.140
    "g_sdisc_b": 8,                # 3.54                0.121
    "g_sdisc_ent_w": 128,          # 34.01               0.081
    "g_sdisc_ent_b": 64,           # 25.69               0.100
    "d_ccls_w": 16,                # 5.77                0.307
    "d_ccls_b": 16,                # 4.81                0.168
    "d_emo_w": 32,                 # 10.30               0.104
    "d_emo_b": 4,                  # 1.63                0.172
    "d_cau_w": 64,                 # 16.78               0.083
    "d_cau_b": 4,                  # 1.89                0.206
    "d_pair_w": 32,                # 11.63               0.134
    "d_pair_b": 8,                 # 2.98                0.311
    "d_dec_w": 32,                 # 12.41               0.164
    "d_dec_b": 32,                 # 15.64               0.113
    "dlat": 128,                   # 44.32               0.041
}
# carel_en_tail_latents / carel_en_tail_backward (rowvec_device.h at K = 768), over FRONT_CASES and FRONT_ODD x grad_out in {none, 2.5}
C_FRONT = {
    "pooled": 128,                 # 33.05               0.009
    "lat": 64,                     # 24.14               0.018
    "d_pooler_w": 32,              # 11.96               0.242
    "d_pooler_b": 32,              # 11.48               0.173
    "dx_last": 64,                 # 21.74               0.029
}


FRONT_MODES = ("dense2", "rows", "dense1")


def front_case(B, Cd, mode, D=24):
    """The latents / backward case of one shape.  "dense2": no cls_rows, seq_len 2, n_rows = 2 B -- the [CLS] stride of the pooler
    input, of the pooler weight gradient, of the dx_last scatter and the B * seq_len zero fill all matter; "dense1": the same at
    seq_len 1; "rows": irregular, increasing cls_rows with n_rows past the last one (seq_len is then unused; it is passed as 2)."""
    assert mode in FRONT_MODES
    return make_front(B, Cd, D, 1 if mode == "dense1" else 2, mode == "rows", seed=B + Cd + FRONT_MODES.index(mode))


FRONT_CASES = [(B, Cd, m) for B in (1, 3, 4, 5, 64, 65, 1024) for Cd in (4, 384, 1024) for m in FRONT_MODES if m != "dense1" or Cd == 384]
# widths that only the losses calls refuse (odd ec_dim, con_dim no multiple of 4, bow_dim 0): latents and backward accept them
FRONT_ODD = (5, 6, "dense2", 23)


def bound(name, scale, table=None):
    c = (C_BOUND if table is None else table)[family(name)]
    return c * U * (scale if torch.is_tensor(scale) else float(scale))


def quantities(ref, scale):
    """(name, ref tensor, scale) per compared quantity; the terms one by one."""
    for k, v in ref.items():
        if k == "pos_weight":
            continue
        if k == "terms":
            for i, n in enumerate(TERM_NAMES):
                yield "term_" + n, v[i], float(scale["terms"][i])
        else:
            yield k, v, scale[k]


def fraction(got, ref, bnd):
    """Worst |got - ref| / bound; a zero bound (an all-zero reference) asks for an exact zero."""
    d = (torch.as_tensor(got).double() - ref.double()).abs()
    bnd = torch.as_tensor(bnd, dtype=torch.float64).expand_as(d) if torch.is_tensor(bnd) else torch.full_like(d, float(bnd))
    f = torch.where(bnd > 0, d / bnd.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    f = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), f)
    return float(f.max())


# ---------------------------------------------------------------------------------------------------------------------------
# the ctypes driver of carel_en_tail_losses / carel_en_tail_losses_bow (torch and the library are imported inside: the CPU tests
# import this module on machines without a GPU)
# ---------------------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 64, -7.25


class EnCall:
    """One prepared call from given latents: every output and the workspace NaN-filled, every output between two guard regions."""

    def __init__(self, c, weighted, label_sum: Optional[float] = None, global_n: int = 0):
        import torch as T
        from carel_vae_amd import _lib as L
        self.L, self.lib, self.c, self.weighted, dev = L, L.load(), c, weighted, "cuda"
        B, V, Cd, D = c.B, c.V, c.Cd, getattr(c, "D", 24)
        self.dims = (B, V, Cd, D)
        ZW = 2 * D + Cd
        self.keep = {k: v.to(dev).contiguous() for k, v in c.P.items()}
        self.inp = {k: getattr(c, k).to(dev).contiguous() for k in ("lat", "eps", "bow", "emo", "cau", "pair")}
        self.dummy = T.zeros(64, device=dev)
        a = self.a = L.EnTailArgs()
        a.batch, a.seq_len, a.hidden, a.ec_dim, a.con_dim, a.bow_dim = B, 1, TH, D, Cd, V
        a.x_last_f32 = a.pooler_w = a.pooler_b = a.pooled = self.dummy.data_ptr()         # read by the latents / backward entry points only
        for i in range(6):
            a.head_w[i] = a.head_b[i] = self.dummy.data_ptr()
        w = lambda k: self.keep[k].data_ptr()      # noqa: E731
        a.cdisc_w, a.cdisc_b, a.ccls_w, a.ccls_b = w("content_disc.weight"), w("content_disc.bias"), w("content_classifier.weight"), w("content_classifier.bias")
        for i, h in enumerate(SMALL):
            a.sdisc_w[i], a.sdisc_b[i] = w(h + ".weight"), w(h + ".bias")
        a.emo_w, a.emo_b, a.cau_w, a.cau_b = w("emotion_classifier.weight"), w("emotion_classifier.bias"), w("cause_classifier.weight"), w("cause_classifier.bias")
        a.pair_w, a.pair_b, a.dec_w, a.dec_b = w("pair_classifier.weight"), w("pair_classifier.bias"), w("decoder.weight"), w("decoder.bias")
        a.emo_labels, a.cau_labels, a.pair_labels, a.bow, a.eps = (self.inp[k].data_ptr() for k in ("emo", "cau", "pair", "bow", "eps"))
        o = c.opt
        a.w_con_adv, a.w_ec_adv, a.w_ecce_adv = o.con_adv_loss_weight, o.ec_adv_loss_weight, o.ecce_adv_loss_weight
        a.w_ec_mul, a.w_con_mul, a.w_pair = o.ec_mul_loss_weight, o.con_mul_loss_weight, o.pair_mul_loss_weight
        a.kl_w_ec, a.kl_w_con = c.kl
        a.label_smoothing, a.epsilon, a.drop_p, a.drop_seed, a.drop_row_offset = o.label_smoothing, o.epsilon, c.drop_p, c.seed, getattr(c, "off", 0)
        if label_sum is not None:
            self.label_sum = T.tensor([label_sum], dtype=T.float32, device=dev)
            a.global_label_sum, a.global_n = self.label_sum.data_ptr(), global_n
        a.lat = self.inp["lat"].data_ptr()
        self.buf, self.shape = {}, {}

        def img(name, shape):
            n = 1
            for s in shape:
                n *= s
            t = T.full((n + 2 * GUARD,), SENTINEL, device=dev)
            t[GUARD:GUARD + n] = float("nan")
            self.buf[name], self.shape[name] = t, tuple(shape)
            return t.data_ptr() + 4 * GUARD
        a.z, a.terms = img("z", (B, ZW)), img("terms", (21,))
        a.work = img("work", (self.lib.carel_en_tail_workspace_floats(B, D, Cd, V),))
        for name, shp in image_shapes(B, V, Cd, D).items():
            p = img(name, shp)
            if name[-1].isdigit():
                getattr(a, name[:-1])[int(name[-1])] = p
            else:
                setattr(a, name, p)
        self.bw = None
        if weighted:
            self.bw = L.EnBowArgs()
            self.bw.work = img("bow_work", (self.lib.carel_en_tail_bow_workspace_floats(B, Cd, V),))

    def view(self, name):
        n = self.buf[name].numel() - 2 * GUARD
        return self.buf[name][GUARD:GUARD + n].reshape(self.shape[name])

    def launch(self):
        """-> the entry point's return code, after a device synchronize."""
        import ctypes as C
        import torch as T
        st = self.L.current_stream()
        if self.weighted:
            rc = self.lib.carel_en_tail_losses_bow(C.byref(self.a), C.byref(self.bw) if self.bw is not None else None, st)
        else:
            rc = self.lib.carel_en_tail_losses(C.byref(self.a), st)
        T.cuda.synchronize()
        return rc

    def guards_intact(self):
        import torch as T
        bad = [k for k, t in self.buf.items() if not (bool(T.all(t[:GUARD] == SENTINEL)) and bool(T.all(t[-GUARD:] == SENTINEL)))]
        assert not bad, "guard regions written: %s" % bad

    def untouched(self):
        """Every output and the workspace still hold their NaN fill (after a refused call)."""
        import torch as T
        self.guards_intact()
        bad = [k for k in self.buf if not bool(T.isnan(self.view(k)).all())]
        assert not bad, "written by a refused call: %s" % bad

    def collect(self, keep_work=False):
        B, V, Cd, D = self.dims
        LW = 2 * Cd + 4 * D
        self.guards_intact()
        out = {k: self.view(k).clone() for k in self.buf if k not in ("work", "bow_work")}
        w, work = carve(B, D, Cd, V), self.view("work")
        out["rowstat"] = work[w["rowstat"]:w["rowstat"] + 8 * B].reshape(4, B, 2)[:3, :, 0].clone()       # the three content heads' sum_j omega bce
        out["dlat"] = work[w["dlat"]:w["dlat"] + B * LW].reshape(B, LW).clone()
        if self.weighted:
            bwk = self.view("bow_work")
            out["xw"] = bwk[:B * Cd].reshape(B, Cd).clone()
            out["con_w"] = bwk[al(B * Cd):al(B * Cd) + B * V].reshape(B, V).clone()
        if keep_work:
            for s, k in enumerate(w["seg_k"]):
                out["xd%d" % s] = work[w["xd"][s]:w["xd"][s] + B * k].reshape(B, k).clone()
        return {k: v.cpu() for k, v in out.items()}


def run_kernel(c, weighted, keep_work=False, **kw):
    """One call of carel_en_tail_losses / carel_en_tail_losses_bow; returns the terms and every image as CPU tensors."""
    call = EnCall(c, weighted, **kw)
    call.L.check(call.launch(), "carel_en_tail_losses_bow" if weighted else "carel_en_tail_losses")
    return call.collect(keep_work)
