#!/usr/bin/env python3
"""One densification pass (clone, split, prune with the Adam moments): the HIP
path (dynamic3dgaussians_amd.densify: plan, one readback, one gather launch)
against the PyTorch formulation (densify_torch: boolean masks, index gathers
and torch.cat) on the same device, at a training run's size:

    colour    P = 300 000, the six reference tensors (17 floats per Gaussian)
    features  the same plus the F = 32 semantic_feature table (49 floats)

40 % of the Gaussians are over the gradient threshold (half of them small
enough to clone, half split), 5 % are below the opacity threshold; i = 500.
Every parameter has both Adam moments.

Each timed run starts from a fresh copy of the parameters and the optimizer
state (untimed) and is bracketed by device events, so a run is the whole pass
as a training loop sees it: kernels, the readback of the four counts, the
allocation of the outputs and the optimizer-state surgery on the host.  The
two implementations alternate, `--runs` times each after `--warmup` runs of
both; the median is reported with the quartiles.  `plan_ms` is
gs_densify_plan with its readback alone.  Each configuration runs in a child
process of its own under a time limit; a child that fails ends the run.  JSON
lines, appended to --out (default profiles/densify/bench.json).

    python tools/densify_bench.py [--runs 25] [--warmup 3] [--points 300000]

Bytes: what the gather must move, from shapes and the pass's own counts: every
source row of every tensor and of both its moments read once (3 x 4 B x width
x P), every output row of the three written once (3 x 4 B x width x P_new),
the three statistics written (12 B x P_new), the flag byte and four ranks of
every Gaussian (17 B x P) and the noise (12 B per row) read.  The share of
8 TB/s is that count over the time of the WHOLE pass, not of the gather
kernel alone.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 8.0e12
CONFIGS = {"colour": 0, "features": 32}
ITERATION = 500
SCENE_RADIUS = 2.0


def _pick(gen, n, ranges, weights, dev):
    import torch
    which = torch.multinomial(torch.tensor(weights, dtype=torch.float32, device=dev), n, replacement=True,
                              generator=gen)
    lo = torch.tensor([r[0] for r in ranges], device=dev)[which]
    hi = torch.tensor([r[1] for r in ranges], device=dev)[which]
    return torch.exp(torch.log(lo) + torch.rand(n, device=dev, generator=gen) * (torch.log(hi) - torch.log(lo)))


def master(P, F, dev):
    """Seeded tensors, moments and statistics; ranges 2 % clear of every threshold."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    smax = _pick(gen, P, [(0.004, 0.019), (0.022, 0.18)], [0.5, 0.5], dev)
    scales = smax[:, None] * (0.3 + 0.7 * torch.rand(P, 3, device=dev, generator=gen))
    scales[:, 0] = smax
    opac = _pick(gen, P, [(0.0005, 0.004), (0.3, 0.95)], [0.05, 0.95], dev)
    tensors = {"means3D": rnd(P, 3), "rgb_colors": torch.rand(P, 3, device=dev, generator=gen),
               "seg_colors": torch.rand(P, 3, device=dev, generator=gen), "unnorm_rotations": rnd(P, 4),
               "logit_opacities": torch.log(opac / (1 - opac))[:, None].contiguous(),
               "log_scales": torch.log(scales)}
    if F:
        tensors["semantic_feature"] = rnd(P, F)
    moments = {k: (0.01 * rnd(*v.shape), 1e-4 * torch.rand(v.shape, device=dev, generator=gen))
               for k, v in tensors.items()}
    denom = torch.randint(1, 12, (P,), device=dev, generator=gen).float()
    g = _pick(gen, P, [(2e-5, 1.6e-4), (2.5e-4, 2e-3)], [0.6, 0.4], dev)
    stats = {"means2D_gradient_accum": g * denom, "denom": denom, "max_2D_radius": torch.rand(P, device=dev) * 40}
    return tensors, moments, stats


def fresh(m):
    """A live (params, variables, optimizer) from the master copy."""
    import torch
    tensors, moments, stats = m
    params = {k: torch.nn.Parameter(v.clone()) for k, v in tensors.items()}
    opt = torch.optim.Adam([{"params": [p], "name": k, "lr": 1e-3} for k, p in params.items()], lr=0.0, eps=1e-15)
    for k, (a, b) in moments.items():
        opt.state[params[k]] = {"step": torch.tensor(10.0), "exp_avg": a.clone(), "exp_avg_sq": b.clone()}
    variables = {k: v.clone() for k, v in stats.items()}
    variables["scene_radius"] = SCENE_RADIUS
    return params, variables, opt


def run_config(name, a):
    import importlib

    import torch
    from dynamic3dgaussians_amd import densify, densify_torch
    D = importlib.import_module("dynamic3dgaussians_amd.densify")
    dev = torch.device("cuda", 0)
    P, F = a.points, CONFIGS[name]
    m = master(P, F, dev)
    sch = D.schedule(ITERATION)
    ws, counts = D.plan(m[2]["means2D_gradient_accum"], m[2]["denom"], m[0]["log_scales"], m[0]["logit_opacities"],
                        grad_thresh=0.0002, clone_max_scale=0.01 * SCENE_RADIUS,
                        prune_min_opacity=sch["remove_threshold"])
    P_new = counts[0] + counts[1] + 2 * counts[3]
    z = torch.randn(2 * counts[2], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    impls = {"hip": densify, "torch": densify_torch}

    def one(fn, timed=True):
        params, variables, opt = fresh(m)
        torch.cuda.synchronize()
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        params, variables = fn(params, variables, opt, ITERATION, accumulate=False, noise=z)
        s1.record()
        torch.cuda.synchronize()
        return s0.elapsed_time(s1), (params, variables, opt)

    out = {}
    for k, fn in impls.items():  # warm-up, and the outputs for the parity check
        for _ in range(a.warmup):
            _, out[k] = one(fn)
    hp, tp = out["hip"][0], out["torch"][0]
    parity = {"rows": [int(hp["means3D"].shape[0]), int(tp["means3D"].shape[0])]}
    assert parity["rows"][0] == parity["rows"][1] == P_new
    for k in hp:
        if k in ("means3D", "log_scales"):
            parity[k + "_max_abs_diff"] = float((hp[k].detach() - tp[k].detach()).abs().max())
        else:
            assert torch.equal(hp[k].detach(), tp[k].detach()), k
        sh, st = out["hip"][2].state[hp[k]], out["torch"][2].state[tp[k]]
        assert torch.equal(sh["exp_avg"], st["exp_avg"]) and torch.equal(sh["exp_avg_sq"], st["exp_avg_sq"]), k
    parity["copied_tensors_and_moments_bit_equal"] = True
    del out, hp, tp
    ms = {k: [] for k in impls}
    for _ in range(a.runs):
        for k, fn in impls.items():
            ms[k].append(one(fn)[0])
    plan_ms = []
    for _ in range(a.runs):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        D.plan(m[2]["means2D_gradient_accum"], m[2]["denom"], m[0]["log_scales"], m[0]["logit_opacities"],
               grad_thresh=0.0002, clone_max_scale=0.01 * SCENE_RADIUS, prune_min_opacity=sch["remove_threshold"])
        s1.record()
        torch.cuda.synchronize()
        plan_ms.append(s0.elapsed_time(s1))
    width = sum(v.numel() // P for v in m[0].values())
    hbm = 3 * 4 * width * (P + P_new) + 12 * P_new + 17 * P + 12 * z.shape[0]
    q = lambda v: [round(x, 4) for x in statistics.quantiles(v, n=4)]  # noqa: E731
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"step": name, "P": P, "F": F, "floats_per_gaussian": width, "iteration": ITERATION,
            "counts": {"kept_originals": counts[0], "kept_clones": counts[1], "split_sources": counts[2],
                       "kept_split_sources": counts[3], "P_new": P_new},
            "over_grad_threshold": round(float((m[2]["means2D_gradient_accum"] / m[2]["denom"] >= 0.0002).float().mean()), 4),
            "runs": a.runs, "warmup": a.warmup,
            "ms_pass": {k: round(v, 4) for k, v in med.items()},
            "ms_pass_quartiles": {k: q(v) for k, v in ms.items()},
            "plan_ms": round(statistics.median(plan_ms), 4),
            "torch_over_hip": round(med["torch"] / med["hip"], 3),
            "hbm_bytes_model": hbm,
            "hbm_model": "gather: 3 x 4 B x floats_per_gaussian x (P + P_new) + 12 B x P_new + 17 B x P + noise",
            "hbm_share_of_8TBps_whole_pass": round(hbm / (med["hip"] * 1e-3) / HBM_BYTES_PER_S, 4),
            "parity_hip_vs_torch_on_device": parity}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "densify", "bench.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if a.child:  # one configuration, in its own process: print its record
        print("RECORD " + json.dumps(run_config(a.child, a)), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--runs", str(a.runs), "--warmup",
               str(a.warmup), "--points", str(a.points)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        recs = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not recs:  # nothing more is started on the device after a failure
            print(f"{step}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return r.returncode or 1
        print(recs[-1], flush=True)
        with open(a.out, "a") as f:
            f.write(recs[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
