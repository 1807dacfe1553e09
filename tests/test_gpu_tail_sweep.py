"""The VAE tail (csrc/tail.hip, rowvec_device.h, mmd_device.h, hsic_device.h) through carel_tail_latents / carel_tail_losses /
carel_tail_backward against oracle.carel_oracle.tail_forward in float64 on the same float32 inputs, over the regimes the host
picks at run time: the batch sizes at which the decoder's sample-group count changes, at which the fused MMD sweep needs a second
trip and at which the 160 KB LDS of the core and decoder kernels is full; every latent width path (ec_dim 24 is compiled in, every
other width runs the run-time-width decoder, the general MMD sweep and the rowvec kernels at N != 96); 1 / 2 / 6 / 8 emotion
logits; MMD / HSIC / no statistic; vocabularies at the 128-entry chunk edges and past 64 chunks; the dead pair head; the
data-parallel hooks (mmd_global_kernel at both widths, partial last chunk and block); an upstream gradient; an extra gradient dz on
the sampled embeddings (carel_tail_backward_dz's dz_extra: tail_add_dz_kernel), alone, beside a scaled loss and beside a loss scaled
by 0, with a log-variance of 6.9 and, through the data-parallel hooks, at a batch of one; carel_scale_f32 on its own.  Every case uses S = 2
(so the [CLS] stride matters), every output starts as NaN, the workspace / dx_last / z / decoder gradients sit between guard
regions, and a second identical run must give the same bits.  Then the refusals of carel_tail_losses: a batch one past the LDS
limit must be refused before anything is launched.

Tolerances are those of tests/test_gpu_tail.py (test_tail_matches_oracle, test_tail_global_batch_hooks), with dx_last scaled per
row.  Every case prints, per quantity, the worst fraction of the bound |got - ref| <= atol + rtol |ref| (1.0 = at the bound) and the
worst |got - ref| / max|ref| (run with -s).  Worst fraction of the bound over the local cases on an MI355X (the dz cases included):
0.11 on pooled, 0.03 on lat / z, 0.03 on every gradient, 0.05 on a dx_last row, below 0.01 on the terms.  (On the CPU the fp32 oracle
itself sits at <= 0.65 of the bound on pooled, <= 0.10 on lat / z, <= 0.03 on every gradient and <= 0.01 on the terms.)
"""
import ctypes as C

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from tests.gpu_util import Guarded
from tests.tail_restate import SCALED_BY_GRAD_OUT, TAIL_KEYS, hip_tail, oracle_tail, setup

pytestmark = pytest.mark.gpu
S, IT, SEED = 2, 7, 31
RT_GRAD, AT_GRAD = 2e-4, 2e-5          # gradients: |got - ref| <= AT_GRAD max|ref| + RT_GRAD |ref| (dx_last: per row)
TERMS = ((1, "mmd"), (2, "emo"), (3, "cau"), (4, "pair"), (5, "kl_e"), (6, "kl_c"), (7, "rec"), (8, "loss"))
ERR_SHAPE = -2

# ---- the batch limits of carel_tail_losses, restated from its host code (csrc/tail.hip).  Both kernels keep the whole batch in the
# 160 KB (40 960 floats) LDS of one CU:
#   core    64 + 64 + 2 * B*2D (z, dz) + 8B + 2B + B*4D (dropout) + 16B + align4(n_hw) + align4(2B) + 2B * (D|1) (MMD rows) + 2B,
#           n_hw = EC*D + EC + D + 1 + 2D + 1 head weights (EC = 6 below)
#   decoder pass 2 = B*2D + 16 + 128 * (2D + 1) + 2 * 128 B (two [B][128] tiles); pass 3 with G sample groups =
#           B*2D + 16 + 128 * (2D + 1) + 128 B + (G - 1) * 128 * (2D + 2); G = 4, halved while pass 3 does not fit or a group would
#           hold fewer than 4 samples
# e.g. ec_dim 24: decoder pass 2 = 304 B + 6288 <= 40960 -> B <= 114; pass 3 at G = 4 = 176 B + 25488 <= 40960 -> B <= 87;
# core = 352 + 270 B + align4(2B) <= 40960 -> B <= 149.
LDS_FLOATS = 160 * 1024 // 4


def core_lds_floats(B, D, EC=6):
    n_hw = EC * D + EC + D + 1 + 2 * D + 1
    return 128 + 2 * B * 2 * D + 8 * B + 2 * B + B * 4 * D + 16 * B + ((n_hw + 3) & ~3) + ((2 * B + 3) & ~3) + 2 * B * (D | 1) + 2 * B


def decoder_plan(B, D):
    """-> (G, floats of the largest pass)."""
    lds0 = B * 2 * D + 16 + 128 * (2 * D + 1) + B * 128
    lds3 = lambda g: lds0 + (g - 1) * 128 * (2 * D + 2)
    G = 4
    while G > 1 and (lds3(G) > LDS_FLOATS or (B + G - 1) // G < 4):
        G >>= 1
    return G, max(lds0 + B * 128, lds3(G))


# ec_dim: (largest batch the decoder accepts, first batch at which G falls back to 2 for LDS reasons or None, largest the core accepts)
# (the core figures are for 6 emotion classes: n_hw moves them by one at most -- 364 / 212 / 149 / 115 with one logit, 363 / 211 / 149 / 114 with 8)
LIMITS = {8: (142, None, 363), 16: (127, None, 211), 24: (114, 88, 149), 32: (101, 38, 115)}


def test_limit_table_follows_from_the_lds_formulas():
    for D, (dec, g2, core) in LIMITS.items():
        assert decoder_plan(dec, D)[1] <= LDS_FLOATS < decoder_plan(dec + 1, D)[1], D
        assert core_lds_floats(core, D) <= LDS_FLOATS < core_lds_floats(core + 1, D), D
        first = next((B for B in range(13, dec + 1) if decoder_plan(B, D)[0] == 2), None)
        assert first == g2, (D, first)
        assert [decoder_plan(B, D)[0] for B in (2, 6, 7, 12, 13)] == [1, 1, 2, 2, 4], D


# ---- cases
def case(B, D=24, EC=6, V=257, dis="mmd", head="ce", p=0.5, allneg=False, grad_out=None, dz=False, lv=0.0):
    """dz: the run gets an extra gradient on the sampled embeddings (make_dz); lv: added to two log-variance biases per side (large_log_var)."""
    return dict(B=B, D=D, EC=EC, V=V, dis=dis, head=head, p=p, allneg=allneg, grad_out=grad_out, dz=dz, lv=lv)


def _cases():
    c = [case(B) for B in (2, 6, 7, 12, 13, 63, 64, 65, 87, 88, 114)]                       # group-count edges, second MMD sweep, the largest
    c += [case(B, D=D) for D in (2, 7, 16, 32) for B in (13, 65)]                           # widths
    c += [case(B, D=32) for B in (37, 38, 101)] + [case(142, D=8), case(127, D=16)]         # G = 4 -> 2 at ec_dim 32; the largest per width
    c += [case(65, D=D, EC=EC) for D in (8, 24) for EC in (2, 8)]                           # CE head with 2 / 8 classes
    c += [case(65, D=D, EC=1, head="bce") for D in (8, 24)]                                 # one-logit BCE head
    c += [case(65, D=8), case(65, D=8, dis="none"), case(65, D=32, dis="none")]             # statistic (mmd at ec_dim 32, B = 65: above)
    c += [case(65, D=D, EC=1, head="bce", dis="hsic") for D in (8, 32)]                     # HSIC with the head of its script
    c += [case(13, D=D, V=V) for D in (24, 32) for V in (2, 127, 128, 129, 8193)]           # chunk edges; 65 chunks: combine's second lane trip
    c += [case(114, V=23771)]
    c += [case(38, D=32, allneg=True), case(38, D=32, allneg=True, p=0.0)]                  # dead pair head, train and eval
    c += [case(13, D=D, grad_out=2.5) for D in (24, 32)]
    # dz_extra: 13 * 48 elements are three blocks of tail_add_dz_kernel with a partial last one, 13 * 14 less than one block
    c += [case(B, dz=True) for B in (13, 65)] + [case(13, D=D, dz=True) for D in (7, 32)]
    c += [case(B, dz=True, grad_out=2.5) for B in (13, 65)] + [case(13, D=D, dz=True, grad_out=0.0) for D in (24, 32)]
    c += [case(13, dz=True, p=0.0), case(13, dz=True, p=0.0, grad_out=2.5)]                 # dropout off
    c += [case(13, dz=True, lv=LV_LARGE, dis="none")]                                       # exp(lv) ~ 1e3: dz * eps * exp(lv) dominates d lat
    return c


def case_id(c):
    s = "B%d-D%d-EC%d-V%d-%s-%s" % (c["B"], c["D"], c["EC"], c["V"], c["dis"], c["head"])
    s += ("-eval" if c["p"] == 0 else "") + ("-allneg" if c["allneg"] else "") + ("-gout" if c["grad_out"] else "")
    return s + ("-gout0" if c["grad_out"] == 0.0 else "") + ("-dz" if c["dz"] else "") + ("-lv" if c["lv"] else "")


LV_LARGE, LV_DIMS = 6.9, (0, 5)          # exp(6.9) = 992


def large_log_var(P, D, lv):
    """lv added to the log-variance biases of the coordinates LV_DIMS of both sides: z is ~1e3 there.  The heads and the decoder get
    zero weights on those coordinates (a probability saturated at 0 or 1 has no finite gradient in the reference's BCE on
    probabilities), so in d lat of those coordinates the routed dz * eps * exp(lv) stands beside the KL term alone."""
    cols = list(LV_DIMS)
    for k in ("emotion_log_var.bias", "cause_log_var.bias"):
        P[k] = P[k].clone()
        P[k][cols] += lv
    for k in ("emotion_classifier.weight", "cause_classifier.weight"):
        P[k] = P[k].clone()
        P[k][:, cols] = 0.0
    for k in ("pair_classifier.weight", "decoder.weight"):
        P[k] = P[k].clone()
        P[k][:, cols + [D + i for i in cols]] = 0.0


def make_dz(B, D, seed, zero_row=1):
    """The extra gradient on [z_e | z_c]: standard normal (both signs), row zero_row all zero (None: no such row)."""
    dz = torch.randn((B, 2 * D), generator=torch.Generator().manual_seed(1000 + seed))
    if zero_row is not None:
        dz[zero_row] = 0.0
    return dz


CASES = _cases()
assert len({case_id(c) for c in CASES}) == len(CASES)


# ---- comparison: |got - ref| <= atol + rtol |ref|, reported as the worst fraction of that bound and the worst error over max|ref|
class Report:
    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def cmp(self, name, got, ref, rtol, atol, scale=None):
        got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        diff = (got - ref).abs()
        atol = torch.as_tensor(atol, dtype=torch.float64)
        frac = float((diff / (atol + rtol * ref.abs())).max())
        den = float(ref.abs().max()) if scale is None else scale
        rel = float(diff.max()) / den if den > 0 else float(diff.max())
        self.rows.append((name, frac, rel))
        if not frac <= 1.0:          # (also catches NaN)
            self.bad.append((name, frac, rel))

    def finish(self):
        print("tail sweep %s: " % self.tag + "  ".join("%s %.2f/%.1e" % r for r in self.rows))
        assert not self.bad, (self.tag, self.bad)


def pin_labels(batch, allneg):
    """labels[0] = 1, labels[1] = 0 (the pos_weight (n - sum y) / sum y is finite and not 0) unless the case is the all-negative one."""
    if not allneg:
        for k in ("labels", "cau_labels"):
            batch[k][0], batch[k][1] = 1.0, 0.0


def bits(t):
    return t.contiguous().view(torch.int32)


def outputs(buf, G):
    return [("pooled", buf.pooled), ("lat", buf.lat), ("z", buf.z), ("terms", buf.terms[:9]), ("dx_last", buf.dx_last)] + [(k, G[k]) for k in TAIL_KEYS]


def check_local(rep, buf, G, ref, B, D, grad_out, rt, at, routed=None):
    """pooled / lat / z / terms / gradients / dx_last of one run against the float64 oracle.  rt / at: the gradient constants (atol is
    at * max|ref|); dx_last per row.  routed: (gradients, d x_last) of grad_out * loss + sum(z * dz) from the oracle, for a run with
    dz_extra: what carel_tail_backward owns (SCALED_BY_GRAD_OUT, dx_last) is held against those as they are; the classifier and decoder
    gradients stay carel_tail_losses' images for grad_out = 1, which dz does not reach."""
    out, pooled, grads, dx = ref
    go = 1.0 if grad_out is None else grad_out
    rep.cmp("pooled", buf.pooled, pooled, 1e-5, 5e-6)
    rep.cmp("lat", buf.lat, torch.cat((out["mu_e"], out["lv_e"], out["mu_c"], out["lv_c"]), dim=1), 1e-5, 1e-5)
    rep.cmp("z", buf.z, torch.cat((out["z_e"], out["z_c"]), dim=1), 1e-5, 2e-5)
    t = buf.terms.cpu()
    for i, k in TERMS:
        rep.cmp(k, t[i], out[k], 1e-4, 1e-5, scale=max(abs(float(out[k])), 1e-30))
    for k in TAIL_KEYS:
        src, f = (routed[0], 1.0) if routed is not None and k in SCALED_BY_GRAD_OUT else (grads, go if k in SCALED_BY_GRAD_OUT else 1.0)
        r = (src[k] if src[k] is not None else torch.zeros_like(G[k].cpu()).double()) * f
        scale = float(r.abs().max()) + 1e-12
        rep.cmp(k, G[k], r, rt, at * scale + 1e-9)
    check_dx(rep, buf.dx_last, dx * go if routed is None else routed[1], B, rt, at)


def check_dx(rep, got, ref, B, rt, at, name="dx_last"):
    got, ref = got.view(B, S, 768), ref.view(B, S, 768)
    assert bool((bits(got[:, 1:]) == 0).all()), "non-[CLS] rows of dx_last must be exact zeros"
    assert bool((ref[:, 1:] == 0).all())
    rowmax = ref[:, 0].abs().amax(dim=1, keepdim=True).double().cpu()
    rep.cmp(name, got[:, 0], ref[:, 0], rt, at * rowmax + 1e-30, scale=float(rowmax.max()))


def run_checked(args, kw, rep):
    """Two identical guarded runs: all finite, identical bits, guards intact.  -> (buf, G) of the first."""
    g = torch.Generator().manual_seed(1234)
    buf, G = hip_tail(*args, guard=g, **kw)
    buf2, G2 = hip_tail(*args, guard=g, **kw)
    for (name, x), (_, y) in zip(outputs(buf, G), outputs(buf2, G2)):
        assert bool(torch.isfinite(x).all()), (rep.tag, name, "not finite")
        assert torch.equal(bits(x), bits(y)), (rep.tag, name, "second run differs")
    for b in (buf, buf2):
        for name, gd in b.guards:
            assert gd.intact(), (rep.tag, name, "guard region written")
    return buf, G


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_tail_sweep(c):
    B, D, V = c["B"], c["D"], c["V"]
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=B + V + D, all_negative=c["allneg"], ec_dim=D, e_num_class=c["EC"],
                                                     disentangle=c["dis"], emotion_head=c["head"])
    pin_labels(batch, c["allneg"])
    if c["lv"]:
        large_log_var(P, D, c["lv"])
    train = c["p"] > 0
    assert c["p"] in (0.0, opt.dropout)
    ref = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, train, SEED, dtype=torch.float64)
    dz = routed = None
    if c["dz"]:
        dz = make_dz(B, D, B + D)
        routed = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, train, SEED, dtype=torch.float64, dz=dz, grad_out=c["grad_out"])[2:]
    if c["lv"]:
        assert all(float(ref[0][k][:, list(LV_DIMS)].exp().median()) > 500 for k in ("lv_e", "lv_c"))
    rep = Report(case_id(c))
    args = (P, x_last, batch, eps_e, eps_c, opt, B, S, V, IT, (c["p"], SEED, 0))
    buf, G = run_checked(args, dict(grad_out=c["grad_out"], dz_extra=dz), rep)
    check_local(rep, buf, G, ref, B, D, c["grad_out"], RT_GRAD, AT_GRAD, routed=routed)
    if c["allneg"]:
        assert float(buf.terms[4]) == 0.0 and not bool(G["pair_classifier.weight"].any()) and not bool(G["pair_classifier.bias"].any())
    if c["dz"] and c["grad_out"] == 0.0:
        # only the routed part survives a loss scaled by 0: with dz = 0 as well, everything carel_tail_backward owns is exactly 0
        # (the classifier and decoder images are not its to scale)
        buf0, G0 = hip_tail(*args, grad_out=0.0, dz_extra=torch.zeros_like(dz))
        for k in SCALED_BY_GRAD_OUT:
            assert bool((G0[k] == 0).all()), (k, "not exactly 0 under grad_out = 0, dz = 0")
        assert bool((buf0.dx_last == 0).all())
        assert bool((G0["decoder.weight"] == G["decoder.weight"]).all()) and bool(G["decoder.weight"].any())
    rep.finish()


@pytest.mark.parametrize("R,Bl,D", [(2, 20, 8), (2, 20, 32), (3, 50, 24)])
def test_tail_sweep_global_batch(R, Bl, D):
    """The data-parallel hooks in the layout of DataParallel.fill_global (each rank's z followed by 16 spare floats, its label sum in
    the first): R shards, rank-averaged gradients and every rank's global statistic against the oracle on the unsharded batch.
    (2, 20, 8): mmd_global_kernel<32> with zero padding, (2, 20, 32) without; (3, 50, 24): 2n = 300 rows, a partial last 256-row
    chunk and a partial last 32-row block."""
    B, V = R * Bl, 257
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=B + V + D, ec_dim=D)
    pin_labels(batch, False)
    ref = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, True, SEED, dtype=torch.float64)
    out, pooled, grads, dx = ref
    rep = Report("global-R%d-B%d-D%d" % (R, Bl, D))
    shards = [({k: v[r * Bl:(r + 1) * Bl] for k, v in batch.items()}, x_last[r * Bl * S:(r + 1) * Bl * S]) for r in range(R)]
    stride = Bl * 2 * D + 16
    packed = torch.full((R, stride), float("nan"), device="cuda")
    for r, (sb, xl) in enumerate(shards):          # pass 1: the latents of each shard -> "all-gather"
        buf, _ = hip_tail(P, xl, sb, eps_e, eps_c, opt, Bl, S, V, IT, (opt.dropout, SEED, r * Bl))
        packed[r, :Bl * 2 * D] = buf.z.reshape(-1)
        packed[r, Bl * 2 * D] = float(sb["labels"].sum())
    tot = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in P.items()}
    terms = torch.zeros(9, dtype=torch.float64)
    z_ref = torch.cat((out["z_e"], out["z_c"]), dim=1)
    for r, (sb, xl) in enumerate(shards):
        kw = dict(global_label_sum=packed.view(-1)[Bl * 2 * D:], global_n=B, global_row_offset=r * Bl, z_global=packed,
                  mmd_grad_scale=float(R), global_rank_stride=stride, global_label_ranks=R)
        buf, G = run_checked((P, xl, sb, eps_e, eps_c, opt, Bl, S, V, IT, (opt.dropout, SEED, r * Bl)), kw, rep)
        sl = slice(r * Bl, (r + 1) * Bl)
        rep.cmp("pooled%d" % r, buf.pooled, pooled[sl], 1e-5, 5e-6)
        rep.cmp("z%d" % r, buf.z, z_ref[sl], 1e-5, 2e-5)
        rep.cmp("mmd%d" % r, buf.terms[1].cpu(), out["mmd"], 3e-5, 2e-6, scale=abs(float(out["mmd"])))      # the global statistic on every rank
        check_dx(rep, buf.dx_last / R, dx[r * Bl * S:(r + 1) * Bl * S], Bl, 3e-4, 3e-5, "dx%d" % r)
        terms += buf.terms[:9].double().cpu() / R
        for k in tot:
            tot[k] += G[k].double().cpu() / R          # gradient averaging over ranks
    for i, k in TERMS[1:]:                             # equal shards: the mean of the ranks' means
        rep.cmp(k, terms[i], out[k], 1e-4, 1e-5, scale=abs(float(out[k])))
    for k in TAIL_KEYS:
        scale = float(grads[k].abs().max()) + 1e-12
        rep.cmp(k, tot[k], grads[k], 3e-4, 3e-5 * scale)
    rep.finish()


@pytest.mark.parametrize("grad_out", [None, 2.5])
def test_tail_sweep_dz_batch_of_one(grad_out):
    """dz_extra at a batch of ONE row.  carel_tail_losses takes such a batch only as one rank's shard of a global batch (its MMD
    divides by n (n - 1)), so the case runs as two ranks of one pair each, in the layout of test_tail_sweep_global_batch, against the
    oracle on the two pairs.  The test averages the ranks' gradients, so each rank routes R x its row of dz; neither row is zero (a
    rank's whole dz would be), so both ranks run tail_add_dz_kernel on data."""
    R, Bl, D, V = 2, 1, 24, 257
    B = R * Bl
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=B + V + D, ec_dim=D)
    pin_labels(batch, False)
    dz = make_dz(B, D, B + D, zero_row=None)
    out, pooled, grads, dx = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, True, SEED, dtype=torch.float64, dz=dz, grad_out=grad_out)
    unit = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, True, SEED, dtype=torch.float64)[2]
    rep = Report("dz-global-R%d-B%d-D%d%s" % (R, Bl, D, "-gout" if grad_out else ""))
    shards = [({k: v[r * Bl:(r + 1) * Bl] for k, v in batch.items()}, x_last[r * Bl * S:(r + 1) * Bl * S]) for r in range(R)]
    stride = Bl * 2 * D + 16
    packed = torch.zeros((R, stride), device="cuda")
    hooks = dict(global_label_sum=packed.view(-1)[Bl * 2 * D:], global_n=B, z_global=packed, mmd_grad_scale=float(R), global_rank_stride=stride,
                 global_label_ranks=R)
    for r, (sb, xl) in enumerate(shards):          # pass 1, for z alone (a batch of one needs the hooks even here; they hold zeros)
        buf, _ = hip_tail(P, xl, sb, eps_e, eps_c, opt, Bl, S, V, IT, (opt.dropout, SEED, r * Bl), global_row_offset=r * Bl, **hooks)
        packed[r, :Bl * 2 * D] = buf.z.reshape(-1)
    for r, (sb, xl) in enumerate(shards):
        packed[r, Bl * 2 * D] = float(sb["labels"].sum())
    tot = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in P.items()}
    for r, (sb, xl) in enumerate(shards):
        kw = dict(hooks, global_row_offset=r * Bl, grad_out=grad_out, dz_extra=R * dz[r * Bl:(r + 1) * Bl])
        buf, G = run_checked((P, xl, sb, eps_e, eps_c, opt, Bl, S, V, IT, (opt.dropout, SEED, r * Bl)), kw, rep)
        check_dx(rep, buf.dx_last / R, dx[r * Bl * S:(r + 1) * Bl * S], Bl, RT_GRAD, AT_GRAD, "dx%d" % r)
        for k in tot:
            tot[k] += G[k].double().cpu() / R
    for k in TAIL_KEYS:
        r = grads[k] if k in SCALED_BY_GRAD_OUT else unit[k]
        rep.cmp(k, tot[k], r, RT_GRAD, AT_GRAD * (float(r.abs().max()) + 1e-12) + 1e-9)
    rep.finish()


# ---- carel_scale_f32
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256, 2048 * 256 + 3])
def test_scale_is_one_rounding(n):
    """x *= s in place with s a device scalar: the bits of torch float32's x * s (one rounding), for s = 0 (signed zeros), 1, 2 and a
    scale that rounds; past 2048 blocks x 256 threads the grid-stride loop takes a second trip; the guard regions around the range
    keep their fill.  Then the refusals: a null range, a null scale and n = 0 return an error and write nothing."""
    lib, st = L.load(), L.current_stream()
    gen = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=gen)
    for s in (0.0, 1.0, 2.0, -0.37):
        g = Guarded((n,), torch.float32, None, gen)
        g.t.copy_(x)
        sd = torch.tensor([s], dtype=torch.float32, device="cuda")
        L.check(lib.carel_scale_f32(g.ptr, n, sd.data_ptr(), st), "carel_scale_f32")
        torch.cuda.synchronize()
        assert g.intact(), (n, s, "guard region written")
        assert torch.equal(bits(g.t.cpu()), bits(x * torch.tensor(s, dtype=torch.float32))), (n, s)
    g = Guarded((n,), torch.float32, None, gen)
    g.t.copy_(x)
    sd = torch.tensor([2.0], dtype=torch.float32, device="cuda")
    for bad in ((None, n, sd.data_ptr()), (g.ptr, n, None), (g.ptr, 0, sd.data_ptr())):
        assert lib.carel_scale_f32(bad[0], bad[1], bad[2], st) != 0
    torch.cuda.synchronize()
    assert g.intact() and torch.equal(bits(g.t.cpu()), bits(x))


# ---- refusals
def _losses_args(B, D, V=257):
    """Arguments of a carel_tail_losses call at batch B after carel_tail_latents has run; -> (args, buffers whose bits a refused call
    must leave alone)."""
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=3, ec_dim=D)
    dev = "cuda"
    W = {k: v.to(dev) for k, v in P.items()}
    G = {k: torch.full_like(v, float("nan")) for k, v in W.items()}
    buf = ops.TailBuffers(B, S, D, opt.e_num_class, V, dev)
    labels = dict(emo=batch["emo_labels"].to(dev).view(-1).contiguous(), cau=batch["cau_labels"].to(dev).view(-1).contiguous(),
                  pair=batch["labels"].to(dev).view(-1).contiguous(), bow=batch["bow_reps"].to(dev).contiguous())
    xl, ee, ec = x_last.to(dev), eps_e.to(dev), eps_c.to(dev)
    a = ops.tail_args(buf, xl, W, labels, ee, ec, opt, ops.kl_anneal_weight(IT, opt), grads=G, drop=(0.5, SEED, 0))
    a._keep = (W, G, labels, xl, ee, ec, buf)
    ops.tail_latents(a)
    torch.cuda.synchronize()
    watched = [("terms", buf.terms), ("z", buf.z), ("work", buf.work)] + [(k, G[k]) for k in TAIL_KEYS[10:]]
    for _, t in watched:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    return a, watched


def _valid_run():
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(8, S, 257, seed=4)
    buf, G = hip_tail(P, x_last, batch, eps_e, eps_c, opt, 8, S, 257, IT, (0.5, SEED, 0))
    return [(n, t.clone()) for n, t in outputs(buf, G)]


# one past the largest batch the decoder accepts (LIMITS, derived above), one past the largest the core kernel accepts, and a batch
# of one without a global batch (the MMD divides by n (n - 1))
REFUSED = [(8, LIMITS[8][0] + 1), (24, LIMITS[24][0] + 1), (32, LIMITS[32][0] + 1), (24, LIMITS[24][2] + 1), (24, 1)]
assert REFUSED == [(8, 143), (24, 115), (32, 102), (24, 150), (24, 1)]


@pytest.mark.parametrize("D,B", REFUSED)
def test_oversize_batch_is_refused_before_anything_is_launched(D, B):
    """CAREL_ERR_SHAPE naming carel_tail_losses; after a device synchronise terms, z, the classifier and decoder gradients and the
    workspace still hold the NaN sentinel bit for bit (a call that forks the loss kernel onto the side stream and then refuses
    leaves that kernel writing them); a valid call before and after gives identical bits."""
    before = _valid_run()
    a, watched = _losses_args(B, D)
    snap = [(n, t.clone()) for n, t in watched]
    rc = L.load().carel_tail_losses(C.byref(a), L.current_stream())
    msg = L.load().carel_last_error().decode()
    torch.cuda.synchronize()          # (every buffer is still alive here: a._keep, watched)
    assert rc == ERR_SHAPE and "carel_tail_losses" in msg, (rc, msg)
    for (n, t), (_, s) in zip(watched, snap):
        assert torch.equal(bits(t), bits(s)), (D, B, n, "written by a refused call")
    after = _valid_run()
    for (n, x), (_, y) in zip(before, after):
        assert torch.equal(bits(x), bits(y)), (n, "a valid call differs after the refused one")
    del a, watched
