"""The tail of the three-space model (csrc/en_tail.hip, rowvec_device.h at K = 768) through the C ABI against the float64 restatement
tests/en_tail_restate.py, at the batch, width and vocabulary edges of its host code:

  carel_en_tail_losses      every output (21 terms, z, the own / second / entropy-share images, classifier and decoder gradients, d lat)
                            at B = 1..9, 63..65 (the 8-wide sample loops, the 4-wide trips), 909 | 910 (the two sides of the 64 KB
                            dynamic-LDS attribute of en_heads_kernel) and 1024; ec_dim 2..64 x con_dim 4..1024 (en_sample_kernel's
                            strided trips, more than 1024 jobs in en_heads_kernel); V at the 64-wide tile, 256-wide split and 2048-wide
                            chunk edges, and V = 16 385, the first vocabulary whose split-K plan has empty slabs (d lat consumes them);
                            a peaked softmax; dropout on with drop_row_offset 0 and 8 and as a shard; the pos_weight override.
  carel_en_tail_losses_bow  the same on a subset, site 120 included.
  carel_en_tail_latents / carel_en_tail_backward   driven directly, per shape: dense x_last at seq_len 2 (the [CLS] stride matters) and
                            irregular cls_rows with n_rows past the last [CLS] row, dense at seq_len 1 for con_dim 384; grad_out null
                            and 2.5, a planted d lat; ec_dim 23 / con_dim 6 / bow_dim 0, which these two entry points accept.
  carel_sgemm_f32, carel_en_pair_logits, carel_axpy_f32 and the refusals of the four entry points.

Every output and the workspace start as NaN, every output sits between guard regions, a second identical call gives the same bits.
Bounds: |got - ref| <= 4 * c * 2^-24 * scale per element, c and scale per quantity as tests/en_tail_restate.py defines and lists them
(c comes from float32 torch on the CPU, never from the kernels).  Every case prints, per quantity, the worst fraction of its bound and
the worst error over max|ref| (run with -s).  Worst over this module on an MI355X: every quantity at most 0.31 of its bound (the table
beside C_BOUND / C_FRONT in the restatement), carel_en_pair_logits below 0.04 of its own.

Three lines of the host / device code that only this module holds in place (read from the code, not tried on a GPU):
  the hipMemsetAsync of the empty slabs in sgemm()   without it slabs nz..splits-1 keep the NaN fill: the split test sees NaN instead of
      zeros, and at V = 16 385 sum_parts_kernel adds slabs 57..63 into dxd_cmul / dz_dec, so every element of d lat is NaN.
  the `b + u < b1` store guard of rowvec_linear_kernel   a trip of four samples would also store the samples past its group's end: for
      the last group those are rows B.. of pooled / lat, i.e. the four-row guard regions behind them (B = 1, 3, 5, 65), for an earlier
      group the next group's first rows, with the clamped row's value.
  the hipFuncSetAttribute call before en_heads_kernel   from B = 910 the launch asks for more than 64 KB of dynamic LDS, which by
      the runtime's contract is rejected at launch time with an error, and check_launch returns it: the B = 910 and 1024 cases fail
      with CarelError, no fault.
"""
import ctypes as C

import pytest
import torch

from carel_vae_amd import _lib as L
from tests import en_tail_restate as T

pytestmark = pytest.mark.gpu
TH = T.TH
NAN = float("nan")


class Report:
    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def cmp(self, name, got, ref, bnd):
        got, ref = torch.as_tensor(got).detach().double().cpu().reshape(ref.shape), ref.detach().double()
        frac = T.fraction(got, ref, bnd)
        den = float(ref.abs().max())
        rel = float((got - ref).abs().max()) / den if den > 0 else float((got - ref).abs().max())
        self.rows.append((name, frac, rel))
        if not frac <= 1.0:          # (also catches NaN)
            self.bad.append((name, frac, rel))

    def finish(self):
        print("en tail sweep %s: " % self.tag + "  ".join("%s %.3f/%.1e" % r for r in self.rows))
        assert not self.bad, (self.tag, self.bad)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def compare_losses(rep, got, ref, scale):
    for name, r, s in T.quantities(ref, scale):
        g = got["terms"][T.TERM_NAMES.index(name[5:])] if name.startswith("term_") else got[name]
        rep.cmp(name, g, r, T.KERNEL_MARGIN * T.bound(name, s))
        if name in ("g_cdisc_w2", "g_cdisc_b2"):          # reported only: the same error on the scale of max|ref| (module docstring of the restatement)
            m = float(r.abs().max())
            rep.rows.append((name + "/max", T.fraction(g.reshape(r.shape), r, T.KERNEL_MARGIN * T.bound(name, m)) if m > 0 else 0.0, 0.0))


def check_losses(c, weighting, ref, scale, tag, **kw):
    weighted = weighting == "bow"
    got, again = T.run_kernel(c, weighted, **kw), T.run_kernel(c, weighted, **kw)
    same_bits(got, again)
    rep = Report(tag)
    compare_losses(rep, got, ref, scale)
    rep.finish()
    return got


@pytest.mark.parametrize("spec", T.PLAIN_CASES, ids=lambda s: s.id)
def test_losses_match_float64(spec):
    ref, scale = T.reference_of(spec, "plain")
    check_losses(T.case_of(spec), "plain", ref, scale, spec.id)


@pytest.mark.parametrize("spec", T.BOW_CASES, ids=lambda s: s.id)
def test_weighted_losses_match_float64(spec):
    ref, scale = T.reference_of(spec, "bow")
    got = check_losses(T.case_of(spec), "bow", ref, scale, spec.id + "-bow")
    assert bool(((got["con_w"] > 0) & (got["con_w"] < 1)).all())
    if spec.p > 0:          # site 120 is a draw of its own
        keep = (got["xw"] != 0).float().mean()
        assert 0.4 < float(keep) < 0.6


def test_shard_at_row_offset_8_is_rows_8_to_15():
    """Rows 8..15 of the 16-row dropout-on problem as an 8-row call at drop_row_offset 8: within bounds of the restatement evaluated
    with that offset, and its ten dropped-out copies are bit for bit rows 8..15 of the 16-row call's (the masks hash the global row)."""
    full = T.case_of(T.Spec(16, 211, 384, p=0.5))
    sh = T.shard(full, 8, 16)
    sh.pair[0], sh.pair[1] = 1.0, 0.0
    assert sh.off == 8 and sh.B == 8
    for wt in ("plain", "bow"):
        ref, scale = T.reference(sh, wt)
        got = check_losses(sh, wt, ref, scale, "shard-8..15-" + wt, keep_work=True)
        whole = T.run_kernel(full, wt == "bow", keep_work=True)
        for s in range(10):
            assert torch.equal(bits(got["xd%d" % s]), bits(whole["xd%d" % s][8:])), s
            assert float((whole["xd%d" % s] == 0).float().mean()) > 0.3
        assert torch.equal(bits(got["z"]), bits(whole["z"][8:]))
        if wt == "bow":
            assert torch.equal(bits(got["xw"]), bits(whole["xw"][8:]))


@pytest.mark.parametrize("weighting", ["plain", "bow"])
def test_pos_weight_override_of_two_half_batches(weighting):
    """Two half batches with global_label_sum / global_n of the whole batch against the restatement with that pos_weight given
    explicitly; everything that does not depend on the pair term is bit-identical to the same shard without the override."""
    full = T.case_of(T.Spec(16, 211, 384, p=0.5))
    halves = [T.shard(full, 0, 8), T.shard(full, 8, 16)]
    halves[1].pair[0], halves[1].pair[1] = 1.0, 0.0
    ysum = float(halves[0].pair.sum() + halves[1].pair.sum())
    pw = (16 - ysum) / ysum
    Cd = full.Cd
    for i, h in enumerate(halves):
        assert (h.B - float(h.pair.sum())) / float(h.pair.sum()) != pw          # the override changes something
        ref, scale = T.reference(h, weighting, pos_weight=pw)
        got = check_losses(h, weighting, ref, scale, "override-half%d-%s" % (i, weighting), label_sum=ysum, global_n=16)
        local = T.run_kernel(h, weighting == "bow")
        for k in got:
            if k not in T.PAIR_DEPENDENT:
                assert torch.equal(bits(got[k]), bits(local[k])), k
        keep = [j for j in range(21) if j not in (6, 16)]
        assert torch.equal(bits(got["terms"][keep]), bits(local["terms"][keep]))
        assert torch.equal(bits(got["dlat"][:, :2 * Cd]), bits(local["dlat"][:, :2 * Cd]))          # the content columns
        assert not torch.equal(got["terms"][16], local["terms"][16]) and not torch.equal(got["d_pair_w"], local["d_pair_w"])
        assert not torch.equal(got["dlat"][:, 2 * Cd:], local["dlat"][:, 2 * Cd:])


# ---------------------------------------------------------------------------------------------------------------------------
# carel_en_tail_latents / carel_en_tail_backward
# ---------------------------------------------------------------------------------------------------------------------------
class FrontCall:
    """pooled / lat / d_pooler_* / dx_last NaN-filled between guard regions of four rows each (a row past the batch lands in them)."""

    def __init__(self, f, V=70):
        self.f, self.V, dev = f, V, "cuda"
        B, Cd, D = f.B, f.Cd, f.D
        self.LW = LW = 2 * Cd + 4 * D
        self.lib = L.load()
        self.keep = dict(x_last=f.x_last.to(dev), pooler_w=f.pooler_w.to(dev), pooler_b=f.pooler_b.to(dev), rows=f.rows.to(dev),
                         head_w=[w.to(dev) for w in f.head_w], head_b=[b.to(dev) for b in f.head_b])
        a = self.a = L.EnTailArgs()
        a.batch, a.seq_len, a.hidden, a.ec_dim, a.con_dim, a.bow_dim = B, f.seq_len, TH, D, Cd, self.V
        a.x_last_f32, a.pooler_w, a.pooler_b = (self.keep[k].data_ptr() for k in ("x_last", "pooler_w", "pooler_b"))
        if f.irregular:
            a.cls_rows, a.n_rows = self.keep["rows"].data_ptr(), f.n_rows
        for i in range(6):
            a.head_w[i], a.head_b[i] = self.keep["head_w"][i].data_ptr(), self.keep["head_b"][i].data_ptr()
        self.buf, self.shape, self.guard = {}, {}, {}
        a.pooled, a.lat = self.img("pooled", (B, TH), 4 * TH), self.img("lat", (B, LW), 4 * LW)
        self.w = T.carve(B, D, Cd, self.V)
        assert self.w["total"] == self.lib.carel_en_tail_workspace_floats(B, D, Cd, self.V)
        a.work = self.img("work", (self.w["total"],), T.GUARD)
        a.d_pooler_w, a.d_pooler_b = self.img("d_pooler_w", (TH, TH), T.GUARD), self.img("d_pooler_b", (TH,), T.GUARD)
        a.dx_last_f32 = self.img("dx_last", (f.n_rows, TH), 4 * TH)

    def img(self, name, shape, guard):
        n = 1
        for s in shape:
            n *= s
        t = torch.full((n + 2 * guard,), T.SENTINEL, device="cuda")
        t[guard:guard + n] = NAN
        self.buf[name], self.shape[name], self.guard[name] = t, shape, guard
        return t.data_ptr() + 4 * guard

    def view(self, name):
        g = self.guard[name]
        return self.buf[name][g:self.buf[name].numel() - g].reshape(self.shape[name])

    def guards_intact(self):
        bad = [k for k, t in self.buf.items() if not (bool(torch.all(t[:self.guard[k]] == T.SENTINEL)) and bool(torch.all(t[-self.guard[k]:] == T.SENTINEL)))]
        assert not bad, "guard regions written: %s" % bad

    def untouched(self):
        self.guards_intact()
        bad = [k for k in self.buf if not bool(torch.isnan(self.view(k)).all())]
        assert not bad, "written by a refused call: %s" % bad

    def latents(self):
        rc = self.lib.carel_en_tail_latents(C.byref(self.a), L.current_stream())
        torch.cuda.synchronize()
        return rc

    def backward(self, grad_out):
        """Plants f.dlat in the workspace where en_carve puts d lat, then the backward call."""
        o = self.w["dlat"]
        self.view("work")[o:o + self.f.B * self.LW] = self.f.dlat.to("cuda").reshape(-1)
        self.g = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device="cuda")
        rc = self.lib.carel_en_tail_backward(C.byref(self.a), None if self.g is None else self.g.data_ptr(), L.current_stream())
        torch.cuda.synchronize()
        return rc

    def run(self, grad_out):
        L.check(self.latents(), "carel_en_tail_latents")
        L.check(self.backward(grad_out), "carel_en_tail_backward")
        self.guards_intact()
        return {k: self.view(k).clone().cpu() for k in ("pooled", "lat", "d_pooler_w", "d_pooler_b", "dx_last")}


def check_front(f, tag, V=70):
    pooled, lat = T.front(f)
    rows = lambda r: r.abs().max(dim=1, keepdim=True).values      # noqa: E731
    other = torch.ones(f.n_rows, dtype=torch.bool)
    other[f.rows.long()] = False
    for go in (None, 2.5):
        got, again = FrontCall(f, V).run(go), FrontCall(f, V).run(go)
        same_bits(got, again)
        ref = T.back(f, go)
        rep = Report("front %s-g%s" % (tag, go))
        bnd = lambda n, s: T.KERNEL_MARGIN * T.bound(n, s, T.C_FRONT)      # noqa: E731
        rep.cmp("pooled", got["pooled"], pooled, bnd("pooled", rows(pooled)))
        rep.cmp("lat", got["lat"], lat, bnd("lat", rows(lat)))
        rep.cmp("d_pooler_w", got["d_pooler_w"], ref["d_pooler_w"], bnd("d_pooler_w", float(ref["d_pooler_w"].abs().max())))
        rep.cmp("d_pooler_b", got["d_pooler_b"], ref["d_pooler_b"], bnd("d_pooler_b", float(ref["d_pooler_b"].abs().max())))
        rep.cmp("dx_last", got["dx_last"], ref["dx_last"], bnd("dx_last", rows(ref["dx_last"])))
        rep.finish()
        assert bool((got["dx_last"][other] == 0).all()) and bool((ref["dx_last"][other] == 0).all())
        assert bool((got["dx_last"][f.rows.long()].abs().sum(dim=1) > 0).all())


@pytest.mark.parametrize("shape", T.FRONT_CASES, ids=lambda s: "B%d-Cd%d-%s" % s)
def test_latents_and_backward_match_float64(shape):
    """Per shape: dense x_last at seq_len 2 (the stride of the pooler input, of its weight gradient, of the dx_last scatter and the
    B * seq_len zero fill), irregular cls_rows with n_rows past the last row, and for con_dim 384 dense at seq_len 1."""
    f = T.front_case(*shape)
    if shape[2] == "dense2":
        assert f.seq_len == 2 and not f.irregular and f.n_rows == 2 * f.B
    if shape[2] == "rows":
        assert f.irregular and f.n_rows > int(f.rows[-1]) + 1
    check_front(f, "B%d-Cd%d-%s" % shape)


def test_latents_and_backward_accept_the_widths_only_the_losses_calls_refuse():
    """An odd ec_dim, a con_dim that is no multiple of 4 and bow_dim 0 are refusals of carel_en_tail_losses(_bow) alone (its float4
    slabs and its vocabulary need them); en_check, which guards all four entry points, asks only for 1 <= ec_dim <= 64 and
    1 <= con_dim <= 1024.  The row-vector kernels of the latents and backward calls take any such width, so these are ACCEPTED there
    (a model with such widths can still predict), and computed within the same bounds."""
    B, Cd, mode, D = T.FRONT_ODD
    check_front(T.front_case(B, Cd, mode, D), "B%d-Cd%d-D%d-V0-%s" % (B, Cd, D, mode), V=0)


# ---------------------------------------------------------------------------------------------------------------------------
# carel_sgemm_f32
# ---------------------------------------------------------------------------------------------------------------------------
def sgemm(A, ta, Bm, tb, Cbuf, ldc, M, N, K, bias=None, acc=0, splits=1, stride=0):
    """A and Bm are the LOGICAL operands [M, K] and [N, K]; they are stored transposed when ta / tb is set."""
    As, Bs = (A.t().contiguous() if ta else A.contiguous()), (Bm.t().contiguous() if tb else Bm.contiguous())
    rc = L.load().carel_sgemm_f32(As.data_ptr(), M if ta else K, ta, Bs.data_ptr(), N if tb else K, tb, Cbuf.data_ptr(), ldc, M, N, K,
                                  None if bias is None else bias.data_ptr(), acc, splits, stride, L.current_stream())
    torch.cuda.synchronize()
    return rc


SG_MN, SG_K = (1, 63, 64, 65, 130), (1, 31, 32, 33, 65)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_sgemm_every_form_exact_on_integers_and_within_the_fmaf_bound(ta, tb):
    """Small-integer data: every product and partial sum is exact in fp32, so the result is bitwise the float64 product.  Random data:
    an fmaf chain of K roundings stays within 2^-24 (K + 1) sum_k |a_k| |b_k|; the bias and the accumulate add are one more rounding
    each, of a partial sum that sum_k |a_k| |b_k| + |bias| + |C| bounds: 2^-24 (K + 1 + n_adds) (sum_k |a_k| |b_k| + |bias| + |C|).  ldc = N + 3:
    the guard columns keep their fill.  Bias, accumulate, both and neither take turns over the shapes."""
    g = torch.Generator().manual_seed(10 * ta + tb)
    n = 0
    for M in SG_MN:
        for N in SG_MN:
            for K in SG_K:
                n += 1
                use_bias, acc = bool(n & 1), (n >> 1) & 1
                for kind in ("int", "rand"):
                    draw = (lambda *s: torch.randint(-3, 4, s, generator=g).float()) if kind == "int" else (lambda *s: torch.randn(s, generator=g))
                    A, Bm, bias, C0 = draw(M, K), draw(N, K), draw(N), draw(M, N)
                    ldc = N + 3
                    Cb = torch.full((M, ldc), T.SENTINEL)
                    Cb[:, :N] = C0 if acc else NAN
                    Cd = Cb.cuda()
                    assert sgemm(A.cuda(), ta, Bm.cuda(), tb, Cd, ldc, M, N, K, bias.cuda() if use_bias else None, acc) == 0
                    out = Cd.cpu()
                    assert bool((out[:, N:] == T.SENTINEL).all()), (M, N, K)
                    extra = (bias.double() if use_bias else 0) + (C0.double() if acc else 0)
                    ref = A.double() @ Bm.double().t() + extra
                    if kind == "int":
                        assert torch.equal(out[:, :N].double(), ref), (M, N, K, use_bias, acc)
                    else:
                        mag = A.double().abs() @ Bm.double().abs().t() + (bias.double().abs() if use_bias else 0) + (C0.double().abs() if acc else 0)
                        assert bool(((out[:, :N].double() - ref).abs() <= T.U * (K + 1 + use_bias + acc) * mag).all()), (M, N, K, use_bias, acc)


@pytest.mark.parametrize("M,N,K,splits", [(5, 52, 70, 7), (65, 130, 65, 4), (3, 8, 16385, 64), (2, 64, 33, 3)])
def test_sgemm_split_slabs_with_empty_chunks_come_back_as_zeros(M, N, K, splits):
    """Fewer non-empty K chunks than slabs asked for: the caller sums `splits` slabs, so the empty ones are zeros, not the NaN fill;
    the non-empty slabs hold their chunk's partial product (exact on integers)."""
    sp, kchunk, nz = T.split_plan(K, splits)
    assert nz < splits
    g = torch.Generator().manual_seed(K)
    A, Bm = torch.randint(-2, 3, (M, K), generator=g).float(), torch.randint(-2, 3, (N, K), generator=g).float()
    for ta, tb in ((0, 1), (0, 0), (1, 1)):
        parts = torch.full((splits * M * N + T.GUARD,), NAN, device="cuda")
        parts[-T.GUARD:] = T.SENTINEL
        assert sgemm(A.cuda(), ta, Bm.cuda(), tb, parts, N, M, N, K, splits=splits, stride=M * N) == 0
        out = parts[:-T.GUARD].cpu().reshape(splits, M, N)
        assert bool((parts[-T.GUARD:] == T.SENTINEL).all())
        for z in range(splits):
            want = A[:, z * kchunk:(z + 1) * kchunk].double() @ Bm[:, z * kchunk:(z + 1) * kchunk].double().t()
            assert torch.equal(out[z].double(), want), (z, nz)
        assert bool((out[nz:] == 0).all()) and torch.equal(out.double().sum(0), A.double() @ Bm.double().t())


def test_sgemm_refusals_leave_the_output_alone():
    M, N, K = 5, 9, 33
    A, Bm, bias = torch.ones(M, K).cuda(), torch.ones(N, K).cuda(), torch.ones(N).cuda()
    Cd = torch.full((4, M, N), NAN, device="cuda")
    lib, st = L.load(), L.current_stream()
    call = lambda a, b, c, m, n, k, bi, acc, sp: lib.carel_sgemm_f32(a, K, 0, b, K, 0, c, N, m, n, k, bi, acc, sp, M * N, st)      # noqa: E731
    p = (A.data_ptr(), Bm.data_ptr(), Cd.data_ptr())
    assert call(*p, M, N, K, bias.data_ptr(), 0, 2) != 0 and b"neither bias nor accumulate" in lib.carel_last_error()
    assert call(*p, M, N, K, None, 1, 2) != 0
    for i in range(3):
        q = list(p)
        q[i] = None
        assert call(*q, M, N, K, None, 0, 1) != 0
    for m, n, k in ((0, N, K), (M, 0, K), (M, N, 0), (-1, N, K), (M, -3, K), (M, N, -2)):
        assert call(*p, m, n, k, None, 0, 1) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(Cd).all())


# ---------------------------------------------------------------------------------------------------------------------------
# carel_en_pair_logits, carel_axpy_f32
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("D", [24, 64])
def test_pair_logits_match_float64(B, D):
    """A lat_stride wider than the row and non-zero offsets.  The kernel is one fmaf chain of 2D terms started from the bias, each term
    w (mu + eps exp(lv)) with three roundings and an expf of its own: |err| <= 2^-24 (2D + 8) (|bias| + sum |w| (|mu| + |eps| exp(lv)))."""
    g = torch.Generator().manual_seed(B + D)
    stride, emo_off, cau_off = 4 * D + 11, 3, 2 * D + 7
    lat = torch.randn(B, stride, generator=g) * 0.3
    eps_e, eps_c = torch.randn(D, generator=g), torch.randn(D, generator=g)
    w, bias = (torch.rand(2 * D, generator=g) * 2 - 1) / (2 * D) ** 0.5, torch.rand(1, generator=g) - 0.5
    out = torch.full((B + 2 * T.GUARD,), T.SENTINEL, device="cuda")
    out[T.GUARD:T.GUARD + B] = NAN
    dev = [t.cuda() for t in (lat, eps_e, eps_c, w, bias)]
    L.check(L.load().carel_en_pair_logits(dev[0].data_ptr(), stride, emo_off, cau_off, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                         dev[4].data_ptr(), B, D, out.data_ptr() + 4 * T.GUARD, L.current_stream()), "carel_en_pair_logits")
    torch.cuda.synchronize()
    assert bool((out[:T.GUARD] == T.SENTINEL).all()) and bool((out[-T.GUARD:] == T.SENTINEL).all())
    l64 = lat.double()
    ze = l64[:, emo_off:emo_off + D], eps_e.double() * l64[:, emo_off + D:emo_off + 2 * D].exp()
    zc = l64[:, cau_off:cau_off + D], eps_c.double() * l64[:, cau_off + D:cau_off + 2 * D].exp()
    we, wc = w[:D].double(), w[D:].double()
    ref = (ze[0] + ze[1]) @ we + (zc[0] + zc[1]) @ wc + bias.double()
    mag = (ze[0].abs() + ze[1].abs()) @ we.abs() + (zc[0].abs() + zc[1].abs()) @ wc.abs() + bias.double().abs()
    err = (out[T.GUARD:T.GUARD + B].cpu().double() - ref).abs()
    print("pair logits B=%d D=%d: worst fraction of the bound %.3f" % (B, D, float((err / (T.U * (2 * D + 8) * mag)).max())))
    assert bool((err <= T.U * (2 * D + 8) * mag).all())


@pytest.mark.parametrize("n", [1, 255, 2048 * 256, 2048 * 256 + 1])
def test_axpy_is_bitwise_the_same_expression(n):
    """Past 2048 blocks x 256 threads the grid-stride loop takes a second trip.  dst = (accumulate ? dst : 0) + s * src: with s a power
    of two or absent, or without accumulate, the expression has ONE rounding however it is compiled and torch float32's `dst + s * src`
    gives its bits.  With accumulate and s = 2.5 the kernel is ONE fused multiply-add (the compiler contracts the expression:
    v_fmac_f32 in axpy_kernel's code), so the same expression in torch is the fused one: the product is exact in float64, the sum is
    rounded there and once more to float32 (no element of these vectors sits at a float32 tie after an inexact first rounding: asserted)."""
    g = torch.Generator().manual_seed(n % 1000)
    src, dst0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    lib, st = L.load(), L.current_stream()
    for acc in (0, 1):
        for s in (None, 0.5, 2.5):
            buf = torch.full((n + 2 * T.GUARD,), T.SENTINEL, device="cuda")
            buf[T.GUARD:T.GUARD + n] = dst0.cuda() if acc else NAN
            sd = None if s is None else torch.tensor([s], dtype=torch.float32, device="cuda")
            sc = src.cuda()
            L.check(lib.carel_axpy_f32(buf.data_ptr() + 4 * T.GUARD, sc.data_ptr(), n, None if sd is None else sd.data_ptr(), acc, st), "carel_axpy_f32")
            torch.cuda.synchronize()
            out = buf.cpu()
            assert bool((out[:T.GUARD] == T.SENTINEL).all()) and bool((out[-T.GUARD:] == T.SENTINEL).all())
            got = out[T.GUARD:T.GUARD + n]
            sv = torch.tensor(1.0 if s is None else s)
            plain = (dst0 if acc else torch.zeros(n)) + sv * src
            if acc and s == 2.5:
                d, pr = dst0.double(), sv.double() * src.double()
                t = d + pr
                fused = t.float()
                bb = t - d
                inexact = ((d - (t - bb)) + (pr - bb)) != 0          # TwoSum: did the float64 add round?
                lo, hi = torch.nextafter(fused, torch.full_like(fused, -float("inf"))), torch.nextafter(fused, torch.full_like(fused, float("inf")))
                tie = (t == (fused.double() + lo.double()) / 2) | (t == (fused.double() + hi.double()) / 2)
                assert not bool((inexact & tie).any())
                assert torch.equal(bits(got), bits(fused)), (acc, s)
                assert n < 255 or not torch.equal(bits(plain), bits(fused))          # the two readings differ on these vectors
            else:
                assert torch.equal(bits(got), bits(plain)), (acc, s)
    for bad in ((None, src.data_ptr(), n), (dst0.data_ptr(), None, n), (dst0.data_ptr(), src.data_ptr(), 0)):
        assert lib.carel_axpy_f32(bad[0], bad[1], bad[2], None, 0, st) != 0          # refused on the host: the CPU pointers are never read


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: an error return before any launch; every NaN-filled output and the workspace untouched
# ---------------------------------------------------------------------------------------------------------------------------
BAD_SHAPES = [("batch", 0), ("batch", 1025), ("ec_dim", 23), ("ec_dim", 66), ("con_dim", 6), ("con_dim", 1028), ("hidden", 512), ("bow_dim", 0)]
# what en_check refuses for all four entry points; an odd ec_dim, a con_dim that is no multiple of 4 and bow_dim 0 are the losses calls'
# own refusals -- the latents and backward calls accept them (test_latents_and_backward_accept_the_widths_only_the_losses_calls_refuse)
BAD_SHAPES_FRONT = [("batch", 0), ("batch", 1025), ("ec_dim", 66), ("con_dim", 1028), ("hidden", 512)]
OPTIONAL = ("cls_rows", "global_label_sum", "d_pooler_w", "d_pooler_b", "dx_last_f32")


def pointer_fields():
    """(field, index or None) of every void* of carel_en_tail_args."""
    for name, tp in L.EnTailArgs._fields_:
        if tp is C.c_void_p:
            yield name, None
        elif isinstance(tp, type) and issubclass(tp, C.Array):
            for i in range(tp._length_):
                yield name, i


def get(a, name, i):
    return getattr(a, name) if i is None else getattr(a, name)[i]


def put(a, name, i, v):
    if i is None:
        setattr(a, name, v)
    else:
        getattr(a, name)[i] = v


@pytest.mark.parametrize("weighted", [False, True], ids=["losses", "losses_bow"])
def test_losses_refusals_touch_nothing(weighted):
    call = T.EnCall(T.case_of(T.Spec(5, 70, 4)), weighted)
    a = call.a
    for name, bad in BAD_SHAPES:
        good = getattr(a, name)
        setattr(a, name, bad)
        assert call.launch() != 0, (name, bad)
        setattr(a, name, good)
    n = 0
    for name, i in pointer_fields():
        if name in OPTIONAL:
            continue
        good = get(a, name, i)
        assert good, (name, i)
        put(a, name, i, None)
        assert call.launch() != 0, (name, i)
        put(a, name, i, good)
        n += 1
    assert n > 70          # every void* of the struct but the five the losses calls do not read
    if weighted:
        good, call.bw.work = call.bw.work, None
        assert call.launch() != 0 and b"null weight scratch" in call.lib.carel_last_error()
        call.bw.work = good
        keep, call.bw = call.bw, None
        assert call.launch() != 0
        call.bw = keep
    call.untouched()
    assert call.launch() == 0          # the same arguments, restored, are accepted
    assert bool(torch.isfinite(call.view("terms")).all())


def test_latents_and_backward_refusals_touch_nothing():
    fc = FrontCall(T.front_case(5, 4, "dense2"))
    a = fc.a
    for entry in (fc.latents, lambda: fc.lib.carel_en_tail_backward(C.byref(a), None, L.current_stream())):
        for name, bad in BAD_SHAPES_FRONT:
            good = getattr(a, name)
            setattr(a, name, bad)
            assert entry() != 0, (name, bad)
            setattr(a, name, good)
    required = [("x_last_f32", None), ("pooler_w", None), ("pooler_b", None), ("pooled", None), ("lat", None)] + \
        [(n, i) for n in ("head_w", "head_b") for i in range(6)]
    for entry, fields in ((fc.latents, required),
                          (lambda: fc.lib.carel_en_tail_backward(C.byref(a), None, L.current_stream()),
                           required + [("work", None), ("dx_last_f32", None), ("d_pooler_w", None), ("d_pooler_b", None)])):
        for name, i in fields:
            good = get(a, name, i)
            put(a, name, i, None)
            assert entry() != 0, (name, i)
            put(a, name, i, good)
    torch.cuda.synchronize()
    fc.untouched()
    assert fc.latents() == 0 and bool(torch.isfinite(fc.view("lat")).all())
