#!/usr/bin/env python3
"""The median-heuristic kernel width: carel_pdist_select for the two median ranks of the squared pairwise distances, at the ECPE
test-set shape (m = 1 938 rows of width 24) and at the row limit (m = 8 192), beside the same quantity through torch on the same GPU
in the same process -- torch.pdist(x).square_() (the N = m (m-1) / 2 distances written out, 134 MB at 8 192 rows) and one
torch.kthvalue per rank, in float32 -- and `latent_independence_test(lat, 1000)` with fixed and with "median" widths.
Timed with device events.  Every part is warmed up; then the parts are run INTERLEAVED, one window of `reps` back-to-back calls each
per round, for `--windows` rounds, and the median window (time per call = window / reps) is reported, so that a disturbance from
other work on the machine hits every part alike.  The peak device memory of each route (above what is allocated before it) is
reported next to its time, and the two routes' values side by side: they differ in the last bits because torch.pdist evaluates
sum (x_i - x_j)^2, not the Gram kernels' n_i + n_j - 2 x_i.x_j.
A one-off build (CAREL_BUILD_TAG / CAREL_EXTRA_FLAGS of carel_vae_amd/build.py, loaded with CAREL_HIP_LIB) can be timed with
--parts select alone: how -DPS_WAVE_AGGREGATE=1 was measured.
Prints one JSON line.   python tools/bench_bandwidth.py [--shapes 1938,8192] [--d 24] [--perms 1000] [--reps 5] [--windows 7] [--parts select,torch,latent]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from carel_vae_amd import _lib as L, drl_classifier as M, ops

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1938,8192", help="rows of the samples, comma separated")
ap.add_argument("--d", type=int, default=24)
ap.add_argument("--scale", type=float, default=3.0, help="standard deviation of the samples' entries")
ap.add_argument("--perms", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5, help="calls per window")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--parts", default="select,torch,latent")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_bandwidth.py needs the GPU: nothing here is measured without one")
want = set(a.parts.split(","))
shapes = [int(s) for s in a.shapes.split(",")]
g = torch.Generator(device="cuda").manual_seed(1)
parts, samples = {}, {}


def median_ranks(m):
    n = m * (m - 1) // 2
    return [(n - 1) // 2, n // 2]


def torch_route(x, ranks):
    d2 = torch.pdist(x).square_()
    return torch.stack([torch.kthvalue(d2, r + 1).values for r in ranks])


for m in shapes:
    x = a.scale * torch.randn((m, a.d), device="cuda", generator=g)
    samples[m] = x
    if "select" in want:
        parts["select_m%d" % m] = (lambda x=x, r=median_ranks(m): ops.pdist_select(x, r), a.reps)
    if "torch" in want:
        parts["torch_m%d" % m] = (lambda x=x, r=median_ranks(m): torch_route(x, r), a.reps)
if "latent" in want:
    m, D_ = shapes[0], a.d
    model = M.DrlClassifier(M.make_opt(pair_bow_dim=8, ec_dim=D_), M.encoder_config("zh", vocab_size=100, layers=1), seed=1).to("cuda").eval()
    mu, lv = (lambda: a.scale * torch.randn((m, D_), device="cuda", generator=g)), (lambda: -1.0 + 0.1 * torch.randn((m, D_), device="cuda", generator=g))
    lat = torch.cat((mu(), lv(), mu(), lv()), 1).contiguous()          # [mu_e | lv_e | mu_c | lv_c], what pair_latents returns
    noise = (torch.randn(D_, device="cuda", generator=g), torch.randn(D_, device="cuda", generator=g))
    perms = M.random_permutations(m, a.perms, "cuda", torch.Generator(device="cuda").manual_seed(2))[1:]
    med = model.latent_independence_test(lat, a.perms, noise=noise, s_e="median", s_c="median", permutations=perms, return_widths=True)
    fixed = (med[2]["s_e"], med[2]["s_c"])         # the same widths as numbers: the two timings differ by the selection alone
    parts["latent_fixed_m%d" % m] = (lambda: model.latent_independence_test(lat, a.perms, noise=noise, s_e=fixed[0], s_c=fixed[1], permutations=perms), a.reps)
    parts["latent_median_m%d" % m] = (lambda: model.latent_independence_test(lat, a.perms, noise=noise, s_e="median", s_c="median", permutations=perms), a.reps)


def window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


for fn, _ in parts.values():           # warm-up: code objects, the allocator's blocks
    fn()
    fn()
torch.cuda.synchronize()
times = {k: [] for k in parts}
for _ in range(a.windows):
    for k, (fn, reps) in parts.items():
        times[k].append(window_ms(fn, reps))

out = dict(d=a.d, scale=a.scale, perms=a.perms, reps=a.reps, windows=a.windows, lib=os.path.basename(L.LIB_PATH))
for k, v in times.items():
    out[k + "_ms"] = round(statistics.median(v), 4)
    out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
for k, (fn, _) in parts.items():
    out[k + "_peak_bytes"] = int(peak_bytes(fn))
for m in shapes:
    x, r = samples[m], median_ranks(m)
    out["workspace_bytes_m%d" % m] = int(L.load().carel_pdist_select_workspace_bytes(m, 2))
    if "select" in want:
        v, c = ops.pdist_select(x, r)
        out["select_values_m%d" % m] = [float(t) for t in v]
        out["select_counts_m%d" % m] = c.tolist()
        if "torch" in want:
            out["torch_values_m%d" % m] = [float(t) for t in torch_route(x, r)]
if "latent" in want:
    out["latent_widths"] = list(fixed)
print(json.dumps(out), flush=True)
