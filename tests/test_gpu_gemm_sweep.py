"""carel_gemm_bf16 of the PRODUCT library over every kernel its plan can pick -- the 128x128 kernel, the 256x192 tile, the 256 x 96n
ping-pong kernel at n = 1, 2, 3, the split-K slab paths of the first and the third with the slab epilogue kernel, and the weight-gradient
(TN) form of each -- against float64 on the kernels' own bf16 / f32 inputs, at the smallest shapes at which each path exists
(tests/gemm_cases.py; tests/test_gemm_cases_host.py asserts from the library's own plan that the table reaches every path).

Every case: inputs and outputs in guarded buffers (tests.gpu_util.Arena), operands exactly as long as their rows (NaN between the rows
of a pitched operand), outputs and workspace NaN before the call and exactly M rows long, guards intact and pad columns still NaN after
it, and a second identical launch gives the same bits.

Exact-grid cases (small integers times powers of two, bias in eighths: every partial sum exact in float32, checked on the host): f32
outputs equal the float64 reference bit for bit, bf16 outputs equal ref.float().to(bfloat16) bit for bit -- ADD_F32, BIAS_BF16,
BIAS_DROP_RESID at p in {0, 0.5}, MUL_BF16 with its colsum_part, the pre-activation of BIAS_GELU, SLAB_F32 slice by slice, colsum_a.
GELU outputs, DGELU and the random-data cases: element by element within the bounds derived in tests/gemm_cases.py (one bf16 rounding,
the erf formula's published error and its fp32 chain, K 2^-24 sum |a||b|).  resid_ln: bit-equal to the same call on
carel_layernorm_fwd's stored rows, and within the LayerNorm forward's per-row bound of float64.

Worst fraction of each bound, stock torch float32 on the CPU | the kernels on an MI355X.  For a bf16 output the CPU figure is taken
before the output's rounding, against the derived part of the bound alone, and the kernel's after it, against the whole bound: the
rounding term is the format's half unit in the last place, which one rounding of anything reaches (0.97 .. 1.00 of it below).
  random data   f32 out, ADD 0.016 | 0.014   DROP_RESID 0.012 | 0.010   slabs 0.012 | 0.008   colsum_a 0.001 | 0.001
                bf16 out, BIAS 0.015 | 0.986   GELU pre-activation 0.006 | 0.968   gelu 0.305 | 0.975   DGELU 0.027 | 0.968, its colsum_part 0.001 | 0.000
  exact grid    gelu (BIAS_GELU, BIAS_GELU_DG) 0.309 | 0.967   gelu' (BIAS_GELU_DG) 0.104 | 0.981   DGELU 0.118 | 0.996, its colsum_part 0.012 | 0.080
  resid_ln      rows 0.245 | 0.245
Every exact-grid output listed above equalled float64 bit for bit on every kernel family, tile width and slab count.

Faults this sweep found, fixed with it:
  * gemm_plan, weight-gradient branch: a (256, 96)-multiple shape that is neither a (128, 128)- nor a (256, 192)-multiple was taken by
    the ping-pong kernel from 64 workgroups on only, and refused below -- with the very split carel_gemm_wgrad_splits proposes (256 x 96,
    T = 8192: 8).  The branch now takes such a shape at any grid, as the row-major-A branch always did (the tn_pp_only_* cases).
  * bf16 outputs / aux with ldc % 8 == 4 were accepted although the 8-column epilogues move 16 bytes per lane: now refused
    (test_refusals); never run.
"""
import ctypes as C

import pytest
import torch

from carel_vae_amd import _lib as L
from tests import gemm_cases as G
from tests.gpu_util import Arena, bits, gemm

pytestmark = pytest.mark.gpu
WORST = {}                   # {bound name: (fraction, case)} over the run; test_report prints it
BF16, F32 = torch.bfloat16, torch.float32


def _record(c, fr):
    for k, f in fr.items():
        key = "%s/%s" % (G.EPI_NAME[c["epi"]] + ("" if c["data"] == "grid" else "_rand"), k)
        if key not in WORST or f > WORST[key][0]:
            WORST[key] = (f, c["name"])


class Run:
    """One case on the device: its buffers, the launch, the outputs' values."""

    def __init__(self, c, d):
        """d: make_inputs(c) (CPU)."""
        self.c, M, N = c, c["M"], c["N"]
        lda, ldb, ldc = G.lds(c)
        self.ldc = ldc
        ar = self.arena = Arena(seed=7)
        self.A, self.B = ar.put(d["A_buf"]), ar.put(d["B_buf"])
        epi, s = c["epi"], c["splits"]
        nan = float("nan")

        def pitched(t, dtype):                  # [M, N] values -> guarded [M, ldc] with NaN pad columns
            full = torch.full((M, ldc), nan, dtype=dtype)
            full[:, :N] = t
            return ar.put(full)

        self.bias = None if d["bias"] is None or epi in (G.DGELU_BF16, G.MUL_BF16, G.ADD_F32, G.SLAB_F32) else ar.put(d["bias"])
        self.resid = self.aux = self.row_map = self.ws = self.stats = self.gamma = self.beta = None
        if c["resid_ln"]:
            self.h = pitched(d["h"], F32)
            self.gamma, self.beta = ar.put(d["gamma"]), ar.put(d["beta"])
            self.stats, self.x32 = ar.nan((M, 2)), ar.nan((M, ldc))
        elif epi in (G.BIAS_DROP_RESID, G.ADD_F32) and d["resid"] is not None:
            self.resid = pitched(d["resid"], F32)
        if epi in (G.DGELU_BF16, G.MUL_BF16):
            self.aux = pitched(d["aux"], BF16)
        if d["row_map"] is not None:
            self.row_map = ar.put(d["row_map"])
        if c["ws_bytes"]:
            self.ws = ar.nan((c["ws_bytes"] // 4,))
        self.out = {}
        if epi == G.SLAB_F32:
            self.out["slabs"] = ar.nan((s, M, ldc))
            if c["colsum_a"]:
                self.out["colsum_a"] = ar.nan((s, M))
        elif epi in G.F32_OUT:
            self.out["out_f32"] = ar.nan((M, ldc))
        else:
            if "out_bf16" not in c["null"]:
                self.out["out_bf16"] = ar.nan((M, ldc), BF16)
            if epi in (G.BIAS_GELU, G.BIAS_GELU_DG):
                self.out["out2_bf16"] = ar.nan((M, ldc), BF16)
            if c["colsum_part"]:
                self.out["colsum_part"] = ar.nan(((M + 127) // 128, N))

    def layernorm(self):
        c = self.c
        L.check(L.load().carel_layernorm_fwd(self.h.ptr, self.gamma.ptr, self.beta.ptr, 1e-12, c["M"], c["N"], self.x32.ptr, None,
                                             self.stats.ptr, L.current_stream()), "carel_layernorm_fwd")

    def launch(self, plain_resid=False):
        c, o = self.c, self.out
        lda, ldb, ldc = G.lds(c)
        t = lambda k: None if k not in o else o[k].t                                      # noqa: E731
        resid = self.resid.t if self.resid is not None else None
        resid_ln = None
        if c["resid_ln"]:
            resid = self.x32.t if plain_resid else self.h.t
            resid_ln = None if plain_resid else (self.stats.t, self.gamma.t, self.beta.t)
        gemm(self.A.t[c["off"]:], self.B.t[c["off"]:], c["form"], c["epi"], c["M"], c["N"], c["K"], splits=c["splits"],
             out_bf16=t("out_bf16"), out2_bf16=t("out2_bf16"), out_f32=t("slabs") if c["epi"] == G.SLAB_F32 else t("out_f32"),
             bias=None if self.bias is None else self.bias.t, resid=resid, aux=None if self.aux is None else self.aux.t, drop=c["drop"],
             lda=lda, ldb=ldb, ldc=ldc, colsum_part=t("colsum_part"), colsum_a=t("colsum_a"), splitk_ws=None if self.ws is None else self.ws.t,
             resid_ln=resid_ln, drop_row_map=None if self.row_map is None else self.row_map.t)
        torch.cuda.synchronize()

    def renan(self):
        for g in self.out.values():
            g.t.fill_(float("nan"))
        if self.ws is not None:
            self.ws.t.fill_(float("nan"))

    def values(self):
        """{output: its [.., :N] columns} after checking the guards and that the pad columns were left alone."""
        assert self.arena.intact(), self.c["name"]
        N, v = self.c["N"], {}
        for k, g in self.out.items():
            if k in ("colsum_part", "colsum_a"):
                v[k] = g.t.clone()
            else:
                assert bool(torch.isnan(g.t[..., N:].float()).all()), (self.c["name"], k, "pad columns written")
                v[k] = g.t[..., :N].clone()
        return v


def to_dev(d):
    return {k: (None if v is None else v.cuda().contiguous()) for k, v in d.items() if not k.endswith("_buf")}


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check_exact(c, got, r):
    for k in G.exact_outputs(c):
        if k not in got:
            continue
        ref = r[k].float()
        ref = ref.to(BF16) if got[k].dtype == BF16 else ref
        if not same_bits(got[k], ref):
            bad = (bits(got[k]) != bits(ref)).nonzero()
            raise AssertionError("%s %s: %d elements differ from float64, first at %r: got %r, want %r" % (
                c["name"], k, bad.shape[0], tuple(bad[0].tolist()), got[k].cpu()[tuple(bad[0])].item(), ref.cpu()[tuple(bad[0])].item()))


@pytest.mark.parametrize("c", [c for c in G.CASES if not c["resid_ln"]], ids=lambda c: c["name"])
def test_case(c):
    d = G.make_inputs(c)
    run = Run(c, d)
    run.launch()
    got = run.values()
    dd = to_dev(d)
    r = G.reference(c, dd)
    check_exact(c, got, r)
    u = None
    if c["epi"] in (G.BIAS_GELU, G.BIAS_GELU_DG) and c["data"] != "grid":
        u = got["out_bf16"].double()                       # random data: the GELU output is judged at the kernel's own pre-activation
        fr = G.worst_fractions(c, dd, {"out_bf16": got["out_bf16"]}, r)
        fr.update({k: v for k, v in G.worst_fractions(c, dd, got, r, u).items() if k != "out_bf16"})
    else:
        fr = G.worst_fractions(c, dd, got, r)
    assert set(fr) | set(G.exact_outputs(c)) >= set(got), (set(got), set(fr))         # every output was judged
    print("%s: %s" % (c["name"], "  ".join("%s %.3f" % kv for kv in sorted(fr.items())) or "exact"))
    _record(c, fr)
    over = {k: v for k, v in fr.items() if not v <= 1.0}
    assert not over, (c["name"], over)
    run.renan()
    run.launch()
    again = run.values()
    for k in got:
        assert same_bits(got[k], again[k]), (c["name"], k, "second launch differs")


@pytest.mark.parametrize("c", [c for c in G.CASES if c["resid_ln"]], ids=lambda c: c["name"])
def test_recomputed_layernorm_residual(c):
    """resid_ln_*: the output is bit-equal to the same call given carel_layernorm_fwd's stored f32 rows as a plain residual, and within
    the LayerNorm forward's per-row bound of the float64 reference taken from the given statistics."""
    d = G.make_inputs(c)
    run = Run(c, d)
    run.layernorm()
    run.launch()
    got = run.values()["out_f32"]
    dd = to_dev(d)
    res = G.resid_ln_rows64(dd, run.stats.t)
    r = G.reference(c, dd, resid_rows=res)
    frac = float(((got.double() - r["out_f32"]).norm(dim=1) / G.resid_ln_row_bound(res, r["out_f32"])).max())
    print("%s: out_f32 rows %.3f" % (c["name"], frac))
    _record(c, {"out_f32_resid_ln_rows": frac})
    assert frac <= 1.0, (c["name"], frac)
    run.renan()
    run.launch(plain_resid=True)
    plain = run.values()["out_f32"]
    assert same_bits(got, plain), c["name"]
    run.renan()
    run.launch()
    assert same_bits(got, run.values()["out_f32"]), c["name"]


# ------------------------------------------------------------------------------------------------ refusals
ERR_ARG, ERR_SHAPE = -1, -2


def test_refusals():
    """Each call the header does not admit returns its error, leaves every NaN-filled output untouched, and the next valid call succeeds."""
    lib = L.load()
    ar = Arena(seed=3)
    n = 512 * 512
    a_bf, b_bf, aux = (ar.put(torch.ones(n, dtype=BF16)) for _ in range(3))
    res, bias, st = ar.put(torch.ones(n)), ar.put(torch.ones(1024)), ar.put(torch.ones(1024))
    o_bf, o2_bf, o_f, cs = ar.nan((n,), BF16), ar.nan((n,), BF16), ar.nan((2 * n,)), ar.nan((4096,))
    NT, NN, TN = G.NT, G.NN, G.TN

    def call(form, epi, M, N, K, splits=1, lda=None, ldb=None, ldc=None, a_off=0, **ptr):
        a = L.GemmArgs()
        a.A, a.B = a_bf.ptr + a_off, b_bf.ptr
        a.lda = lda if lda is not None else (M if form == TN else K)
        a.ldb = ldb if ldb is not None else (K if form == NT else N)
        a.ldc = ldc if ldc is not None else N
        a.M, a.N, a.K, a.form, a.epilogue, a.splits = M, N, K, form, epi, splits
        full = dict(out_bf16=o_bf.ptr, out2_bf16=o2_bf.ptr, out_f32=o_f.ptr, bias=bias.ptr, resid_f32=res.ptr, aux_bf16=aux.ptr)
        full.update(ptr)
        for k, v in full.items():
            setattr(a, k, v)
        return lib.carel_gemm_bf16(C.byref(a), L.current_stream())

    B, GL, DG, DR, DGE, ADD, SL, MUL = G.BIAS_BF16, G.BIAS_GELU, G.BIAS_GELU_DG, G.BIAS_DROP_RESID, G.DGELU_BF16, G.ADD_F32, G.SLAB_F32, G.MUL_BF16
    refused = [
        ("M = 100 with N = 128", ERR_SHAPE, lambda: call(NT, B, 100, 128, 256)),
        ("ragged M with K = 192", ERR_SHAPE, lambda: call(NT, B, 300, 96, 192)),
        ("ragged M, N = 96, DGELU with colsum_part", ERR_SHAPE, lambda: call(NN, DGE, 300, 96, 256, colsum_part=cs.ptr)),
        ("K not a multiple of 64", ERR_SHAPE, lambda: call(NT, B, 128, 128, 96)),
        ("TN, K % (64 splits) != 0 off the ping-pong kernel", ERR_SHAPE, lambda: call(TN, SL, 128, 128, 320, splits=2)),
        ("splits > 1 with a non-slab epilogue", ERR_ARG, lambda: call(NT, B, 128, 128, 256, splits=2)),
        ("NN + GELU", ERR_ARG, lambda: call(NN, GL, 128, 128, 256)),
        ("NT + DGELU", ERR_ARG, lambda: call(NT, DGE, 128, 128, 256)),
        ("TN + bias", ERR_ARG, lambda: call(TN, B, 128, 128, 256)),
        ("BIAS_BF16 without out_bf16", ERR_ARG, lambda: call(NT, B, 128, 128, 256, out_bf16=None)),
        ("BIAS_GELU without out2_bf16", ERR_ARG, lambda: call(NT, GL, 128, 128, 256, out2_bf16=None)),
        ("BIAS_GELU_DG without out_bf16", ERR_ARG, lambda: call(NT, DG, 128, 128, 256, out_bf16=None)),
        ("BIAS_GELU_DG without out2_bf16", ERR_ARG, lambda: call(NT, DG, 128, 128, 256, out2_bf16=None)),
        ("BIAS_DROP_RESID without out_f32", ERR_ARG, lambda: call(NT, DR, 128, 128, 256, out_f32=None)),
        ("BIAS_DROP_RESID without resid_f32", ERR_ARG, lambda: call(NT, DR, 128, 128, 256, resid_f32=None)),
        ("DGELU without out_bf16", ERR_ARG, lambda: call(NN, DGE, 128, 128, 256, out_bf16=None)),
        ("DGELU without aux_bf16", ERR_ARG, lambda: call(NN, DGE, 128, 128, 256, aux_bf16=None)),
        ("MUL without out_bf16", ERR_ARG, lambda: call(NN, MUL, 128, 128, 256, out_bf16=None)),
        ("MUL without aux_bf16", ERR_ARG, lambda: call(NN, MUL, 128, 128, 256, aux_bf16=None)),
        ("ADD_F32 without out_f32", ERR_ARG, lambda: call(NN, ADD, 128, 128, 256, out_f32=None)),
        ("SLAB_F32 without out_f32", ERR_ARG, lambda: call(TN, SL, 128, 128, 256, out_f32=None)),
        ("colsum_a on NT", ERR_ARG, lambda: call(NT, B, 128, 128, 256, colsum_a=cs.ptr)),
        ("two of the three resid_ln pointers", ERR_ARG, lambda: call(NT, DR, 128, 128, 256, resid_ln_stats=st.ptr, resid_ln_gamma=st.ptr)),
        ("resid_ln off BIAS_DROP_RESID", ERR_ARG, lambda: call(NT, ADD, 128, 128, 256, resid_ln_stats=st.ptr, resid_ln_gamma=st.ptr, resid_ln_beta=st.ptr)),
        ("a misaligned A", ERR_ARG, lambda: call(NT, B, 128, 128, 256, a_off=8)),
        ("lda % 8 != 0", ERR_ARG, lambda: call(NT, B, 128, 128, 256, lda=260)),
        ("ldb % 8 != 0", ERR_ARG, lambda: call(NN, B, 128, 128, 256, ldb=132)),
        ("ldc % 4 != 0", ERR_ARG, lambda: call(NT, ADD, 128, 128, 256, ldc=130)),
        ("bf16 output with ldc % 8 == 4", ERR_ARG, lambda: call(NT, B, 128, 128, 256, ldc=132)),
        ("bf16 outputs with ldc % 8 == 4 (GELU)", ERR_ARG, lambda: call(NT, DG, 128, 128, 256, ldc=132)),
        ("bf16 aux with ldc % 8 == 4", ERR_ARG, lambda: call(NN, MUL, 128, 128, 256, ldc=132)),
    ]
    for what, code, f in refused:
        assert f() == code, (what, lib.carel_last_error())
    assert b"ldc a multiple of 8" in lib.carel_last_error()
    torch.cuda.synchronize()
    assert ar.intact()
    for o in (o_bf, o2_bf, o_f, cs):
        assert bool(torch.isnan(o.t.float()).all())
    assert call(NT, B, 128, 128, 256, bias=None) == 0            # the next valid call succeeds: 256 ones times ones
    torch.cuda.synchronize()
    assert ar.intact() and bool((o_bf.t[:128 * 128].float() == 256).all()) and bool(torch.isnan(o_bf.t[128 * 128:].float()).all())


def test_report():
    """(runs last in this module) the worst fraction of every bound over the cases that ran: the module docstring's record."""
    print("MI355X, worst fraction of each bound: " + "  ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))
