#!/usr/bin/env python3
"""Benchmark: rendered Mpix/s of the differentiable Gaussian rasterizer, fwd+bwd.

Workload (BASELINE.json configs[2], the north-star metric's config): a
Panoptic-sized scene of 300k Gaussians rendered from a 27-camera rig at
800x800 (G3 call pattern of dyn_train.py:244: precomputed colours +
32-channel semantic features + label), forward AND backward for every camera,
then ONE flat all-reduce of the per-Gaussian gradients (N > 1) and an Adam
step -- one step of the per-timestep training loop.  With features (camera
batch mode, N > 1) the features' all-reduce and Adam step run on a side
stream behind the next step's projection and binning, whose blend waits for
them (gs_gaussians.feature_ready; GS_BENCH_OVERLAP=0: in line; at one rank
GS_BENCH_OVERLAP=1 overlaps the feature Adam step the same way); the timed
region ends after they do.  Data is synthetic (no
network): seeded Gaussians and cameras (dynamic3dgaussians_amd/scene.py,
camera.py).

Two call patterns (--mode; the headline is --mode, the other one is timed
right after it on the same scene and reported as `other_mode`):
  batch   the rank's cameras through GaussianRasterizerBatch: one launch per
          stage for all of them, gradients summed over the cameras in-kernel
          (the default: the multi-camera step as one pass);
  percam  one drop-in GaussianRasterizer call per camera (the reference's
          call pattern) over 4 HIP streams, gradients summed by a
          GradientSink.

Scaling (headline: weak): every rank renders its own 27 cameras of a 27*N
camera rig with the full Gaussian set replicated; value = all ranks' pixels /
step time.  `--cams-total T` makes the headline the north star's step split
across the ranks instead (BASELINE.json configs[3], strong scaling): ONE rig
of T cameras split over the ranks (--split windows, the default: the first
N * (T // N) cameras whole, c mod N, the T % N left over cut into bands of
tile rows that even out the ranks' work (tile-list instances per row from
a probe forward of the rig, a fixed cost per extra camera piece) -- image
sharding, gs_camera tile_*, distributed.shard_camera_windows, DESIGN.md 6.2;
--split cameras: camera c on rank c mod N, distributed.shard_cameras), each rank
renders its share as one batch, then the gradient all-reduce and Adam;
value = T cameras' pixels / step time.  At N > 1 the weak headline is
followed by the same measurement of the 27-camera split step, reported as
`split_step` (so one driver run gives both curves).

    python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line (rank 0).  A plain run does what the headline needs and
no more: set-up, W warm-up steps and the one untimed step that `--full` times
per stage (so both kinds of run time the same steps), K timed steps, the line
with the contract
fields (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`)
and the run's `config`.  `--dump-outputs DIR`: after the timed steps, one more
step of the timed path from the seeded parameters the run started with, and
what it computed written to DIR (dump_outputs).  Everything else is measured
only with `--full`: the per-stage timing and the instance counts, the
other call pattern, the split step and the CPU legs.  With `--full` the line
also carries
`roofline` (dominant kernel, live HIP-event timing over the timed region),
`cpu_baseline` (north star's naive pure-PyTorch fp32 CPU splat, fwd + autograd
bwd, on a bounded tile sample of camera 0, on the host's cores; the
single-thread C oracle beside it as `cpu_baseline.c_oracle`; rank 0 at N=1
only) and `psnr_vs_oracle_db` (the rendered image of camera 0 vs the
oracle's).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from dynamic3dgaussians_amd import _lib  # noqa: E402
from dynamic3dgaussians_amd.camera import camera_rig  # noqa: E402
from dynamic3dgaussians_amd.distributed import (GradBucket, ShardedStep, rank_load_scale, shard_camera_windows,  # noqa: E402
                                                shard_cameras)
from dynamic3dgaussians_amd.optim import FusedAdam  # noqa: E402
from dynamic3dgaussians_amd.rasterizer import (GaussianRasterizationSettings,  # noqa: E402
                                               GaussianRasterizer, GaussianRasterizerBatch, GradientSink)
from dynamic3dgaussians_amd.scene import make_gaussians  # noqa: E402

METRIC = "rendered Mpix/s fwd+bwd (1/8 GPU) at 300k Gaussians; PSNR vs ref"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--cams", type=int, default=27, help="cameras per rank per step (weak scaling)")
    ap.add_argument("--cams-total", type=int, default=0,
                    help="strong scaling: one rig of this many cameras split over the ranks (see --split)")
    ap.add_argument("--split", default="windows", choices=["cameras", "windows"],
                    help="strong-scaling split: work-balanced with image sharding of the left-over cameras "
                         "(windows, the default) or whole cameras c mod N (cameras)")
    ap.add_argument("--balance", default="measured", choices=["model", "measured"],
                    help="window split: cut by the work model alone, or re-cut once from every rank's measured "
                         "step per modelled unit (distributed.rank_load_scale)")
    ap.add_argument("--whole-scale", default="",
                    help="comma-separated measured-feedback factors (a split_model.whole_scale of an earlier run): "
                         "use them instead of measuring, so every proxy rank cuts the same windows")
    ap.add_argument("--proxy-world", type=int, default=0,
                    help="one GPU standing in for rank --proxy-rank of an N-rank --cams-total split: the "
                         "rank's own cameras and windows, no collective (the per-rank shape)")
    ap.add_argument("--proxy-rank", type=int, default=0)
    ap.add_argument("--cpu-tiles", type=int, default=20,
                    help="CPU baseline sample: a TxT block of 16x16 tiles at the centre of camera 0")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--compat", default="reference", choices=["reference", "fixed"])
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without its CPU legs")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: per-stage timing and the roofline of the dominant kernel, instance "
                         "counts, the other call pattern, the split step, the CPU baselines and the PSNR legs")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps: one more step of the timed path from the seeded parameters the run "
                         "started with (the same inputs every run); rank 0 writes what it computed to "
                         "DIR/<name>.npy (float32): the rendered images, depths, features and radii and the "
                         "parameters' gradients; arrays above their share of 48 MB as a fixed seeded sample")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dump-params", default="",
                    help="rank 0 writes the parameters after the timed steps to this .npz (rehearsal checks)")
    ap.add_argument("--step-times", action="store_true",
                    help="also report host timestamps of the timed steps (diagnostic)")
    ap.add_argument("--sub-batches", type=int, default=int(os.environ.get("GS_BENCH_SUB_BATCHES", "1")),
                    help="batch mode: the rank's cameras as this many camera batches (round robin) on their own "
                         "HIP streams, so one batch's binning and launch tails overlap another's blend kernels")
    ap.add_argument("--mode", default=os.environ.get("GS_BENCH_MODE", "batch"), choices=["batch", "percam"],
                    help="batch: the rank's cameras through GaussianRasterizerBatch (one launch per stage "
                         "for all of them); percam: one GaussianRasterizer call per camera (the drop-in)")
    return ap.parse_args()


def setup_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal knobs for a one-GPU box (never used by the driver's runs):
    # GS_BENCH_BACKEND=gloo with GS_BENCH_SHARE_GPU=1 puts every rank on
    # cuda:0 and exchanges the gradient bucket over gloo.
    backend = os.environ.get("GS_BENCH_BACKEND", "nccl")
    dev_index = 0 if os.environ.get("GS_BENCH_SHARE_GPU") == "1" else local
    # GS_BENCH_FORCE_DIST=1 (one-GPU rehearsal of the RCCL calls: RCCL refuses
    # two ranks on one device): a process group even at WORLD_SIZE 1
    if world > 1 or os.environ.get("GS_BENCH_FORCE_DIST") == "1":
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
    return world, rank, torch.device("cuda", dev_index if world > 1 else 0)


def make_params(args, dev):
    """Dynamic3DGaussians parameterisation (dyn_train.py:117-129, helpers.py:98-107)."""
    g = make_gaussians(args.gaussians, F=args.features, seed=args.seed)
    params = {
        "means3D": g["means3D"],
        "rgb_colors": g["colors"],
        "unnorm_rotations": g["rotations"],
        "logit_opacities": torch.logit(g["opacities"]),
        "log_scales": torch.log(g["scales"]),
    }
    if args.features:
        params["semantic_feature"] = g["semantic_feature"]
    params = {k: v.to(dev).requires_grad_(True) for k, v in params.items()}
    label = torch.ones(args.gaussians, device=dev)
    return params, label


def params2rendervar(params, label):
    rv = {
        "means3D": params["means3D"],
        "colors_precomp": params["rgb_colors"],
        "rotations": torch.nn.functional.normalize(params["unnorm_rotations"]),
        "opacities": torch.sigmoid(params["logit_opacities"]),
        "scales": torch.exp(params["log_scales"]),
        # screen-space means: the bench does no densification, so no gradient
        # is requested for them (GradientSink / batch keep the statistics)
        "means2D": torch.zeros_like(params["means3D"]),
        "label": label,
    }
    if "semantic_feature" in params:
        rv["semantic_feature"] = params["semantic_feature"]
    return rv


def raw_rendervar(params, label, means2D):
    """params2rendervar's inputs for GaussianRasterizerBatch(raw_params=True):
    the raw parameters themselves, activated inside the preprocess kernels
    (sigmoid / exp / normalize, GS_FLAG_ACTIVATE); means2D is a placeholder
    (the batch keeps the densification statistics itself)."""
    rv = {"means3D": params["means3D"], "colors_precomp": params["rgb_colors"],
          "rotations": params["unnorm_rotations"], "opacities": params["logit_opacities"],
          "scales": params["log_scales"], "means2D": means2D, "label": label}
    if "semantic_feature" in params:
        rv["semantic_feature"] = params["semantic_feature"]
    return rv


# One more camera piece costs a rank its projection and binning launches and
# launch tails.  Measured in isolation (tools/piece_cost.py: the same pixels
# of one camera as 1 / 2 / 3 pieces): 0.152 of a camera's step time (51 vs
# 337 us; profiles/r05pc/piece_cost.json).  In the split itself the ranks
# holding a second left-over camera's piece ran 0.058 ms above the others at
# equal modelled load (the second piece is another camera's projection and
# plan; profiles/r05px: 1.403-1.406 vs 1.30-1.38 ms), i.e. about 0.32 of a
# camera per piece: the model charges that.  (A model of every camera's
# measured one-camera step instead of its tile-list instances did not predict
# the batched ranks better, 1.30-1.45 ms, and varied run to run:
# profiles/r05px2.)
PIECE_FRACTION = 0.32


def split_shard(n_cams, rank, world, how, W, H, costs=None, whole_scale=None):
    """[(camera, tile window or None)] of `rank` in a `world`-rank split of an
    n_cams rig (--split; windows balanced by `costs` = (row_cost, piece_cost),
    rig_costs, and the measured-feedback factors `whole_scale`)."""
    if how == "cameras":
        return [(c, None) for c in shard_cameras(n_cams, rank, world)]
    row_cost, piece = costs if costs is not None else (None, 0.0)
    return shard_camera_windows(n_cams, rank, world, (W + 15) // 16, (H + 15) // 16, row_cost=row_cost,
                                piece_cost=piece, whole_scale=whole_scale)


def shard_model_load(shard, costs, gy, whole_scale=1.0):
    """The modelled load of a rank's shard in row_cost units (its rows plus
    the fixed cost of every piece; whole cameras' rows times `whole_scale`,
    as shard_camera_windows weighs them)."""
    row_cost, piece = costs
    load = 0.0
    for c, w in shard:
        rows = range(gy) if w is None else range(w[1], w[3])
        load += sum(row_cost[c][y] for y in rows) * (whole_scale if w is None else 1.0) + piece
    return load


def time_shard(shard, rig, params, label, args, dev, steps=20, warmup=8):
    """Forward + backward ms per step of one rank's camera batch (the split
    step's rendering work; the Adam step is the same on every rank)."""
    W_, H_, F = args.width, args.height, args.features
    sets = make_settings([rig[c] for c, _ in shard], dev, args.compat, None,
                         [w for _, w in shard] if any(w is not None for _, w in shard) else None)
    ras = GaussianRasterizerBatch(sets, raw_params=True)
    n = len(shard)
    g = torch.Generator(device=dev).manual_seed(5)
    ups = [torch.randn(n, 3, H_, W_, device=dev, generator=g), torch.randn(n, 1, H_, W_, device=dev, generator=g),
           torch.randn(n, F, H_, W_, device=dev, generator=g) if F else None]
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    m2 = torch.zeros_like(params["means3D"])

    def one():
        for v in leaves.values():
            v.grad = None
        rv = raw_rendervar(leaves, label, m2)
        if F:
            im, _, feat, depth, _ = ras(**rv)
            torch.autograd.backward([im, depth, feat], ups)
        else:
            im, _, depth, _ = ras(**{k: v for k, v in rv.items() if k != "semantic_feature"})
            torch.autograd.backward([im, depth], ups[:2])
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measured_balance(n_cams, world, rank, rig, params, label, args, dev, costs, iters=2):
    """Measured-feedback balancing of the window split (--balance measured):
    every rank's shard of the current cut is timed (all of them in this
    process for a --proxy-world rank; each rank its own, gathered, in a
    distributed run), each rank's whole-camera load is rescaled by its
    measured step per modelled unit (distributed.rank_load_scale), and the
    windows are cut again -- `iters` times, the factors compounding.
    Returns (whole_scale, every round's per-rank ms)."""
    gy = (args.height + 15) // 16
    ws = [1.0] * world
    rounds = []
    for _ in range(iters):
        shards = [split_shard(n_cams, r, world, "windows", args.width, args.height, costs, ws) for r in range(world)]
        model = [shard_model_load(sh, costs, gy, ws[r]) for r, sh in enumerate(shards)]
        if dist.is_initialized() and dist.get_world_size() > 1:
            cdev = dev if dist.get_backend() == "nccl" else torch.device("cpu")  # gloo rehearsals: host tensors
            t = torch.tensor([time_shard(shards[rank], rig, params, label, args, dev)], dtype=torch.float64,
                             device=cdev)
            allt = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(allt, t)
            ms = [float(x.item()) for x in allt]
        else:
            ms = [time_shard(sh, rig, params, label, args, dev) for sh in shards]
        rounds.append(ms)
        ws = [w * f for w, f in zip(ws, rank_load_scale(ms, model))]
    return ws, rounds


def rig_costs(rig, params, label, args, dev):
    """The work model of --split windows: per camera and tile row the
    instances of the row's tile lists (rig_row_costs), and the fixed cost of
    one more camera piece, PIECE_FRACTION of a mean camera's instances.
    Returns (row_cost, piece_cost)."""
    rows = rig_row_costs(rig, params, label, args, dev)
    return rows, PIECE_FRACTION * sum(sum(r) for r in rows) / len(rows)


def rig_row_costs(rig, params, label, args, dev):
    """The work model of --split windows: per camera of `rig` and tile row,
    the instances of the row's tile lists (one forward per camera, the tile
    ranges read back with gs_debug_export).  Every rank computes the same."""
    from dynamic3dgaussians_amd import _C
    L_ = _lib.load()
    W, H = args.width, args.height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    P = params["means3D"].shape[0]
    out = []
    with torch.no_grad():
        rv = params2rendervar(params, label)
        for s in make_settings(rig, dev, args.compat):
            o = _C.rasterize_gaussians_batch(
                s.bg, rv["means3D"], rv["colors_precomp"], None, rv["opacities"], rv["scales"], rv["rotations"],
                1.0, torch.Tensor([]), s.viewmatrix.reshape(1, 16), s.projmatrix.reshape(1, 16), [s.c_x], [s.c_y],
                [s.tanfovx], [s.tanfovy], H, W, torch.Tensor([]), 0, s.campos.reshape(1, 3), False, False,
                compat=args.compat)
            rg = torch.zeros(gx * gy, 2, dtype=torch.int32, device=dev)
            _lib.check(L_.gs_debug_export(P, W, H, o[6].data_ptr(), None, o[8].data_ptr(), 0, None, None, None,
                                          None, None, None, rg.data_ptr(), None,
                                          torch.cuda.current_stream(dev).cuda_stream), "tile ranges")
            r = rg.cpu().numpy().view(np.uint32).reshape(gy, gx, 2).astype(np.int64)
            out.append((r[..., 1] - r[..., 0]).sum(1).tolist())
    return out


def make_settings(cams, dev, compat, sink=None, windows=None):
    out = []
    for i, c in enumerate(cams):
        out.append(GaussianRasterizationSettings(
            image_height=c.H, image_width=c.W, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
            c_x=c.c_x, c_y=c.c_y, bg=torch.zeros(3, device=dev), scale_modifier=1.0,
            viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(dev),
            projmatrix=torch.from_numpy(c.projmatrix.copy()).to(dev), sh_degree=0,
            campos=torch.from_numpy(c.campos.copy()).to(dev), prefiltered=False, debug=False,
            confidence=None, compat=compat, grad_sink=sink,
            tile_window=None if windows is None else windows[i]))
    return out


def stage_bytes(L, Pv, P, W, H, F, compat, cams, C=3, TB=128):
    """Algorithmic HBM bytes per camera and stage (restated
    for this build's kernels) in a launch of `cams` cameras: per-Gaussian
    inputs and outputs shared by the launch's cameras count once per launch
    (1/cams per camera).  TB = binning workgroups per camera (gs_common.h
    TB_BLOCKS); K = 1 (precomputed colours).  Reference numerics never read
    the feature rows in the blend backward (their term of dL/dalpha is dead,
    Q5; gs_render.hip FIXED_FEAT): no 4F per instance there."""
    npix = W * H
    T = ((W + 15) // 16) * ((H + 15) // 16)
    feat_bwd = 4 * F if compat == "fixed" else 0
    return {
        # means, scales, rotations, opacity, colours in (+ the 3D covariance out)
        # once per launch; per camera radii, render record, tile count, rect out
        "preprocess": P * (56 + 24) / cams + P * (4 + 64 + 4 + 16),
        "scan": 16 * P + 3 * 4 * TB * T + 12 * T,      # rect records in, block-tile counts, ranges
        "duplicate": 16 * P + 4 * TB * T + 8 * L,      # rect records, block offsets, (depth, id) keys out
        "sort": 8 * L + 4 * L,                          # per-tile sort: keys in, ids out
        "ranges": 8 * T + 16 * T,                       # dispatch records from the ranges
        "render_fwd": L * (4 + 8 + 16 + 4 * C + 4 + 4 * F) + npix * 4 * (C + F + 2 + 1),
        "render_bwd": L * (4 + 8 + 16 + 4 * C + 4) + L * feat_bwd + npix * 4 * (C + F + 4 + 1)
        + Pv * 4 * (3 + 4 + 1 + C + F + 1),
        # per launch: means, scales, rotations, 3D covariance, opacity in and the
        # 7 gradient outputs (92 B) out; per camera the accumulation record,
        # radius and conic
        "preprocess_bwd": P * (72 + 92) / cams + P * (40 + 4 + 20),
    }


def pmc_for(workload):
    """The committed rocprofv3 PMC summaries (profiles/pmc_traffic.json,
    pmc_valu.json, pmc_atomic.json: tools/gpu_pmc.sh) -- only when they were
    measured on this bench line's exact workload (the record's `workload`
    block); per-camera counts of another scene or rig say nothing about this
    one.  Returns {name: summary} of the matching files."""
    out = {}
    for name in ("traffic", "valu", "atomic"):
        try:
            with open(os.path.join(REPO, "profiles", f"pmc_{name}.json")) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        if d.get("workload") == workload:
            out[name] = d
    return out


# stage -> (kernel key in profiles/pmc_valu.json, matrix-core cycles per MFMA)
# matrix-core cycles per MFMA on one SIMD (MI355X_MICROARCH.md constants):
# v_mfma_f32_16x16x32_bf16 16 (backward), v_mfma_f32_32x32x16_bf16 32 (forward)
VALU_KERNEL = {"render_bwd": ("render_bwd", 16), "render_fwd": ("render_fwd", 32),
               "sort": ("tile_sort", 0), "preprocess": ("preprocess_fwd", 0), "preprocess_bwd": ("preprocess_bwd", 0)}
SIMDS, CLOCK_GHZ, VALU_ISSUE_CYC = 1024, 2.4, 4  # MI355X: 256 CUs x 4 SIMDs; wave64 VALU = 4 cycles
ATOMIC_PEAK_GBS = 1300.0  # chip-wide float-atomic rate, MI355X_MICROARCH.md "Global float atomics"


def issue_view(pmc, stage, avg_ms, cams):
    """VALU + matrix-core issue cycles of a kernel (matching PMC counts per
    camera x the launch's cameras) over the SIMD-cycles of its live launch time."""
    try:
        key, mfma_cyc = VALU_KERNEL[stage]
        k = {c: v * cams for c, v in pmc["valu"]["kernels"][key].items()}
    except (KeyError, TypeError):
        return None
    cyc = k["SQ_INSTS_VALU"] * VALU_ISSUE_CYC + k.get("SQ_INSTS_MFMA", 0) * mfma_cyc
    avail = SIMDS * CLOCK_GHZ * 1e9 * avg_ms * 1e-3
    return {"valu_insts_per_launch": int(k["SQ_INSTS_VALU"]), "mfma_insts_per_launch": int(k.get("SQ_INSTS_MFMA", 0)),
            "issue_cycles_per_launch": int(cyc), "frac": round(cyc / avail, 4),
            "peak": f"{SIMDS} SIMDs x {CLOCK_GHZ} GHz, {VALU_ISSUE_CYC} cycles per wave64 VALU instruction"}


def atomic_view(pmc, stage, avg_ms, cams):
    """Memory-side float-atomic traffic of a kernel (matching PMC 64-B request
    counts per camera x the launch's cameras) over its live launch time,
    against the chip-wide float-atomic rate."""
    try:
        req = pmc["atomic"]["requests_per_camera"][stage] * cams
    except (KeyError, TypeError):
        return None
    if not req or avg_ms <= 0:
        return None
    gbs = req * pmc["atomic"].get("bytes_per_request", 64) / (avg_ms * 1e-3) / 1e9
    return {"requests_per_launch": int(req), "achieved": round(gbs, 1), "peak": ATOMIC_PEAK_GBS, "unit": "GB/s",
            "frac": round(gbs / ATOMIC_PEAK_GBS, 4)}


def stage_table(stage_ms, alg_per_cam, pmc, cams):
    """Per-stage HBM roofline of one step: algorithmic bytes (the 8(d) model)
    and, with matching PMC counts, measured HBM bytes (FETCH_SIZE x 2 +
    WRITE_SIZE, tools/pmc_traffic.py) over the stage's device time."""
    meas = (pmc.get("traffic") or {}).get("bytes_per_camera", {})
    out = {}
    for st, ms in stage_ms.items():
        if ms <= 0 or st not in alg_per_cam:
            continue
        row = {"ms": round(ms, 4), "alg_bytes": int(alg_per_cam[st] * cams)}
        row["alg_frac"] = round(row["alg_bytes"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        if st in meas:
            b = meas[st] * cams
            row["hbm_bytes"] = int(b)
            row["hbm_GBs"] = round(b / (ms * 1e-3) / 1e9, 1)
            row["hbm_frac"] = round(b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        out[st] = row
    return out


def calc_psnr(img1, img2):
    """The reference's PSNR (external.py:84-86: per-channel MSE over the
    pixels, 20 log10(1/sqrt(mse))), averaged over the channels as its callers
    do (train.py report / visualize)."""
    a = np.asarray(img1, np.float64).reshape(img1.shape[0], -1)
    b = np.asarray(img2, np.float64).reshape(img2.shape[0], -1)
    mse = ((a - b) ** 2).mean(1)
    with np.errstate(divide="ignore"):
        return float(np.mean(20 * np.log10(1.0 / np.sqrt(mse))))


DUMP_BUDGET_BYTES = 48 << 20  # all of --dump-outputs' files together (float32 elements)


def dump_outputs(path, calls, params, seed, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: what one step of the timed path handed its caller, as
    path/<name>.npy (float32, flattened).  `calls` are the step's rasterizer
    calls in order ({image, radii, depth, feature}: one camera batch, or one
    entry per camera of the per-camera drop-in); their outputs are joined
    along the camera axis.  Beside them the gradient the step left on every
    parameter (grad_<name>, where the step binds one).  The parameters after
    the optimizer step are not written: Adam's moments come from the timed
    steps, whose gradients differ from run to run by the float atomics' order,
    so its update of the restored parameters is not the same every run.  Every
    array gets the same share of `budget`; a larger one is written as a
    sample of its elements at sorted indices drawn from a generator seeded by
    (seed, the array's position), so two runs with the same arguments write
    the same elements."""
    arrays = {}
    for name in ("image", "depth", "feature", "radii"):
        parts = [c[name] if c[name].dim() == 4 or name == "radii" and c[name].dim() == 2 else c[name][None]
                 for c in calls if c[name] is not None]
        if parts:
            arrays[name] = torch.cat([p.detach() for p in parts])
    for k, v in params.items():
        if v.grad is not None:
            arrays["grad_" + k] = v.grad.detach()
    os.makedirs(path, exist_ok=True)
    share = budget // 4 // len(arrays)
    for i, (name, t) in enumerate(arrays.items()):
        flat = t.reshape(-1)
        if flat.numel() > share:
            idx = np.sort(np.random.default_rng([seed, i]).integers(0, flat.numel(), share))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        np.save(os.path.join(path, name + ".npy"), flat.float().cpu().numpy())


def host_cores():
    """The host cores this process may use: the scheduler's affinity set,
    capped by OMP_NUM_THREADS when set (the GPU box exports its CPU share
    there; os.cpu_count() shows the whole machine)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS")
    if omp and omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def torch_cpu_splat(args, params0, cam, img_hip, up):
    """North star's CPU baseline: a naive pure-PyTorch splat (oracle/torch_splat.py,
    fp32 dense per-tile algebra, projection as utils/graphics_utils.py:51-74
    sets it up) of the same scene and camera, forward + autograd backward
    through the same activations as the step (sigmoid / exp / normalize), on
    the host's cores, over a bounded sample: the --cpu-tiles^2 tiles at the
    image centre (every Gaussian is projected; only the sampled tiles blend)."""
    from oracle import torch_splat as TS
    cores = host_cores()
    prev = torch.get_num_threads()
    torch.set_num_threads(cores)
    try:
        gx, gy = (cam.W + 15) // 16, (cam.H + 15) // 16
        n = max(1, min(args.cpu_tiles, gx, gy))
        tx0, ty0 = (gx - n) // 2, (gy - n) // 2
        tiles = [(tx0 + i, ty0 + j) for j in range(n) for i in range(n)]
        leaf = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in params0.items()}
        view = torch.from_numpy(cam.viewmatrix.copy()).float()
        proj = torch.from_numpy(cam.projmatrix.copy()).float()
        t0 = time.perf_counter()
        color, depth, feat, _ = TS.render(
            leaf["means3D"], leaf["rgb_colors"], torch.sigmoid(leaf["logit_opacities"]),
            torch.exp(leaf["log_scales"]), torch.nn.functional.normalize(leaf["unnorm_rotations"]), view, proj,
            cam.tanfovx, cam.tanfovy, cam.c_x, cam.c_y, cam.W, cam.H, torch.zeros(3),
            features=leaf.get("semantic_feature"), tiles=tiles)
        t1 = time.perf_counter()
        uc, ud, uf = up
        loss = (color * uc).sum() + (depth * ud).sum()
        if feat is not None:
            loss = loss + (feat * uf).sum()
        loss.backward()
        t2 = time.perf_counter()
    finally:
        torch.set_num_threads(prev)
    ys = slice(ty0 * 16, min((ty0 + n) * 16, cam.H))
    xs = slice(tx0 * 16, min((tx0 + n) * 16, cam.W))
    a = color.detach().numpy()[:, ys, xs].astype(np.float64)
    b = img_hip[:, ys, xs].astype(np.float64)
    mse = float(np.mean((a - b) ** 2))
    npix = (ys.stop - ys.start) * (xs.stop - xs.start)
    return {"value": round(npix / 1e6 / (t2 - t0), 5), "unit": "Mpix/s", "cores": cores, "kind": "port",
            "sample": f"camera 0, the {n}x{n} tiles ({npix} px) at the image centre of {cam.W}x{cam.H}; "
                      f"{args.gaussians} Gaussians projected, F={args.features}; fwd {t1 - t0:.2f}s + "
                      f"autograd bwd {t2 - t1:.2f}s; oracle/torch_splat.py fp32 on {cores} threads",
            "psnr_vs_hip_db": round(10 * np.log10(1.0 / mse), 2) if mse > 0 else "inf"}


def cpu_baseline(args, params, label, cam, settings, dev):
    """The CPU baselines on camera 0 of the same scene: north star's naive
    PyTorch splat (torch_cpu_splat, the reported `cpu_baseline`) and the C
    oracle (plain C restatement, 1 thread, the whole camera, forward +
    backward: `cpu_baseline.c_oracle`).  Also returns the PSNR of the HIP
    render of the same camera against the oracle's, and both renders' PSNR
    against a ground-truth image (the oracle's render of the scene with its
    means jittered by N(0, 0.002), seeded: a stand-in for a training target)."""
    from oracle import oracle as O
    with torch.no_grad():
        rv = params2rendervar(params, label)
        host = {k: v.detach().float().cpu() for k, v in rv.items() if isinstance(v, torch.Tensor)}
    t0 = time.perf_counter()
    L, color, feat, depth, alpha, radii, st = O.rasterize_gaussians(
        np.zeros(3, np.float32), host["means3D"], host["colors_precomp"],
        host.get("semantic_feature"), host["opacities"], host["scales"], host["rotations"], 1.0,
        None, cam.viewmatrix, cam.projmatrix, cam.c_x, cam.c_y, cam.tanfovx, cam.tanfovy, cam.H,
        cam.W, None, 0, cam.campos, compat=args.compat)
    t1 = time.perf_counter()
    rng = np.random.default_rng(1)
    dc = rng.standard_normal((3, cam.H, cam.W), dtype=np.float32)
    df = rng.standard_normal((args.features, cam.H, cam.W), dtype=np.float32)
    dd = rng.standard_normal((1, cam.H, cam.W), dtype=np.float32)
    da = np.zeros((1, cam.H, cam.W), np.float32)
    cam4 = (cam.tanfovx, cam.tanfovy, cam.c_x, cam.c_y) if args.compat == "reference" else \
        (cam.c_x, cam.c_y, cam.tanfovx, cam.tanfovy)
    O.rasterize_gaussians_backward(
        np.zeros(3, np.float32), host["means3D"], radii, host["colors_precomp"],
        host.get("semantic_feature"), host["scales"], host["rotations"], 1.0, None, cam.viewmatrix,
        cam.projmatrix, *cam4, dc, df, dd, da, None, 0, cam.campos, st, L, None, None, alpha,
        compat=args.compat)
    t2 = time.perf_counter()
    # HIP render of the same camera
    with torch.no_grad():
        rv = params2rendervar(params, label)
        out = GaussianRasterizer(settings)(**rv)
        torch.cuda.synchronize()
    img = out[0].float().cpu().numpy()
    mse = float(np.mean((img.astype(np.float64) - color.astype(np.float64)) ** 2))
    psnr = float("inf") if mse == 0 else 10 * np.log10(1.0 / mse)
    g = torch.Generator().manual_seed(7)
    jitter = host["means3D"] + 0.002 * torch.randn(host["means3D"].shape, generator=g)
    gt = O.rasterize_gaussians(
        np.zeros(3, np.float32), jitter.contiguous(), host["colors_precomp"], host.get("semantic_feature"),
        host["opacities"], host["scales"], host["rotations"], 1.0, None, cam.viewmatrix, cam.projmatrix,
        cam.c_x, cam.c_y, cam.tanfovx, cam.tanfovy, cam.H, cam.W, None, 0, cam.campos,
        compat=args.compat)[1]
    p_hip, p_ref = calc_psnr(img, gt), calc_psnr(color, gt)
    psnr_gt = {"hip": round(p_hip, 4), "oracle": round(p_ref, 4), "delta_db": round(p_hip - p_ref, 6),
               "gt": "oracle render of the scene with means jittered by N(0, 0.002)",
               "formula": "external.py:84-86 calc_psnr, channel mean"}
    mpix = cam.W * cam.H / 1e6
    c_oracle = {"value": round(mpix / (t2 - t0), 4), "unit": "Mpix/s", "cores": 1, "kind": "port",
                "sample": f"the whole camera 0 ({cam.W}x{cam.H}, {args.gaussians} Gaussians, F={args.features}), "
                          f"fwd {t1 - t0:.2f}s + bwd {t2 - t1:.2f}s, oracle/gs_oracle.c single thread"}
    up = (torch.from_numpy(dc), torch.from_numpy(dd), torch.from_numpy(df) if args.features else None)
    cb = torch_cpu_splat(args, params, cam, img, up)
    cb["c_oracle"] = c_oracle
    return cb, psnr, psnr_gt


def other_mode(mode, has_windows, strong, world, enabled=True):
    """The call pattern timed beside the headline (the per-camera drop-in
    or the camera batch), or None.  The per-camera drop-in renders whole
    cameras only, and the decision must be the same on every rank (the other
    mode's steps hold collectives): a split's ranks differ in whether they
    hold a window, so a split over N > 1 ranks skips it on all of them."""
    if not enabled or has_windows or (strong and world > 1):
        return None
    return "percam" if mode == "batch" else "batch"


def main():
    args = parse()
    if os.environ.get("GS_BENCH_TRACEBACKS"):
        # debugging a stuck run: every thread's Python stack to stderr every N s
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["GS_BENCH_TRACEBACKS"]), repeat=True, file=sys.stderr)
    # The bench line is the only output on stdout: native libraries may print
    # there (RCCL writes a version banner on rank 0 when the communicator
    # comes up), so fd 1 goes to stderr for the run and the line is written
    # to the saved descriptor.
    sys.stdout.flush()
    line_fd = os.dup(1)
    os.dup2(2, 1)
    world, rank, dev = setup_dist(args)
    dist_on = dist.is_initialized()
    _lib.load()
    torch.manual_seed(args.seed)

    strong = args.cams_total > 0
    my_windows = None
    params, label = make_params(args, dev)
    if args.proxy_world and (world > 1 or not strong):
        raise SystemExit("--proxy-world stands in for one rank of a --cams-total split on ONE process")
    if strong:
        # the north star's step: one rig split over the ranks (--split)
        s_rank, s_world = (args.proxy_rank, args.proxy_world) if args.proxy_world else (rank, world)
        if args.split == "cameras" and args.cams_total < s_world:
            raise SystemExit(f"--cams-total {args.cams_total} < {s_world} ranks")
        rig = camera_rig(args.cams_total, args.width, args.height, seed=args.seed)
        costs = rig_costs(rig, params, label, args, dev) if args.split == "windows" else None
        wscale, first_ms = None, None
        if args.whole_scale:
            wscale = [float(x) for x in args.whole_scale.split(",")]
            if len(wscale) != s_world:
                raise SystemExit(f"--whole-scale needs {s_world} factors")
        elif args.split == "windows" and args.balance == "measured" and s_world > 1:
            wscale, first_ms = measured_balance(args.cams_total, s_world, s_rank, rig, params, label, args, dev,
                                                costs)
        shard = split_shard(args.cams_total, s_rank, s_world, args.split, args.width, args.height, costs, wscale)
        my_cams = [rig[c] for c, _ in shard]
        if any(w is not None for _, w in shard):
            my_windows = [w for _, w in shard]
    else:
        rig = camera_rig(args.cams * world, args.width, args.height, seed=args.seed)
        my_cams = rig[rank * args.cams:(rank + 1) * args.cams]
    # The per-camera gradients of a step are summed inside the backward
    # kernels (GradientSink: GS_FLAG_ACCUMULATE into per-stream buffers)
    # instead of autograd adding 7 gradient tensors per camera into the
    # leaves; GS_BENCH_SINK=0 restores autograd's accumulation.
    # (one camera: nothing to sum -- the per-camera step is then exactly the
    # reference's train.py iteration: activations, render, backward, Adam)
    use_sink = os.environ.get("GS_BENCH_SINK", "1") != "0" and len(my_cams) > 1
    sink = GradientSink() if use_sink else None
    settings = make_settings(my_cams, dev, args.compat, sink, my_windows)
    # the CPU-baseline / PSNR leg renders the initial scene (independent of the
    # optimizer steps taken by warmup and timing)
    params0 = {k: v.detach().clone() for k, v in params.items()}
    # The reference's Adam (train.py:119-135).  Default: FusedAdam, one HIP
    # launch, bit-identical to torch.optim.Adam (tests/test_optim.py);
    # GS_BENCH_OPTIM=torch / torch_fused selects torch's own kernels.
    groups = [
        {"params": [params["means3D"]], "lr": 1.6e-4, "name": "means3D"},
        {"params": [params["rgb_colors"]], "lr": 2.5e-3, "name": "rgb_colors"},
        {"params": [params["unnorm_rotations"]], "lr": 1e-3, "name": "unnorm_rotations"},
        {"params": [params["logit_opacities"]], "lr": 0.05, "name": "logit_opacities"},
        {"params": [params["log_scales"]], "lr": 1e-3, "name": "log_scales"},
    ] + ([{"params": [params["semantic_feature"]], "lr": 1e-3, "name": "semantic_feature"}]
         if args.features else [])
    optim_kind = os.environ.get("GS_BENCH_OPTIM", "fused_hip")

    def make_opt(gs):
        if optim_kind == "fused_hip":
            return FusedAdam(gs, lr=0.0, eps=1e-15)
        return torch.optim.Adam(gs, lr=0.0, eps=1e-15, fused=optim_kind == "torch_fused")

    # N > 1, camera batches, F > 0: the feature gradients (32 of the 46 floats
    # per Gaussian) are all-reduced behind the next step -- their all-reduce and
    # Adam update run on a side stream while the next step projects and bins,
    # and that step's blend waits for the update (gs_gaussians.feature_ready);
    # only the geometry gradients are exchanged on the step's critical path.
    # Double-buffered feature gradients: step k writes buffer k % 2 while the
    # exchange of step k-1 still reads the other.  GS_BENCH_OVERLAP=0: one
    # bucket, exchanged before Adam; =force: overlapped at a world of one too
    # (rehearses the RCCL async all-reduce + side-stream wait on one GPU).
    ov_env = os.environ.get("GS_BENCH_OVERLAP", "1")
    overlap = (dist_on and args.features > 0 and args.mode == "batch"
               and ((world > 1 and ov_env != "0") or ov_env == "force"))
    # One rank, no process group: nothing to exchange, but the feature Adam
    # step (32 of the 46 floats per Gaussian) still runs on the side stream
    # behind the next step's projection and binning, gated the same way.
    local_overlap = (not dist_on and args.features > 0 and args.mode == "batch"
                     and os.environ.get("GS_BENCH_OVERLAP", "0") == "1")
    split_opt = overlap or local_overlap
    # The camera batch takes the raw parameters and applies params2rendervar's
    # activations in its preprocess kernels (GS_FLAG_ACTIVATE: ~20 fewer
    # elementwise launches per step; tests/test_gpu_raw_params.py holds it to
    # the torch-activation step); GS_BENCH_RAW=0 keeps torch's activations.
    raw = os.environ.get("GS_BENCH_RAW", "1") != "0"
    # The camera batch as one rank of N (N > 1, or a --proxy-world stand-in):
    # Adam sharded over the ranks (distributed.ShardedStep over ShardedAdam, ZeRO stage 1) --
    # reduce-scatter, Adam on the rank's 1/N of the parameters, all-gather --
    # with the backward writing its gradients straight into the exchange
    # buffer (grad_into).  GS_BENCH_ZERO=0: the all-reduce + full Adam on
    # every rank; =force: also at a world of one with a process group (the
    # RCCL reduce-scatter / all-gather rehearsal on one GPU).
    zero_env = os.environ.get("GS_BENCH_ZERO", "1")
    zero = (args.mode == "batch" and raw and zero_env != "0"
            and (world > 1 or args.proxy_world > 1 or (zero_env == "force" and dist_on)))
    z_rank, z_world = (args.proxy_rank, args.proxy_world) if args.proxy_world else (rank, world)
    if zero:
        # the package's sharded step (distributed.ShardedStep): with `overlap`
        # geometry in line, features behind the next step (two gradient buffers)
        lrs = {g_["name"]: g_["lr"] for g_ in groups}
        z_coll = dist_on and (world > 1 or zero_env == "force")
        zs = ShardedStep(params, lrs, rank=z_rank, world=z_world, eps=1e-15, collectives=z_coll, overlap=overlap)
    elif split_opt:
        opt = make_opt([g_ for g_ in groups if g_["name"] != "semantic_feature"])
        opt_feat = make_opt([g_ for g_ in groups if g_["name"] == "semantic_feature"])
    else:
        opt = make_opt(groups)
    # N > 1: every parameter's .grad is a view into the all-reduce bucket, so
    # the backward accumulates straight into it (no pack/unpack copies) and
    # one fill clears it.  N = 1 has no exchange: gradients stay unbound, so
    # autograd hands the backward's tensors to the leaves without the six
    # accumulate kernels and the fill (-0.06 ms per step).
    if zero:
        pass
    elif overlap:
        bucket = GradBucket({k: v for k, v in params.items() if k != "semantic_feature"}, bind_grads=True)
        feat_buckets = [GradBucket({"semantic_feature": params["semantic_feature"]}, bind_grads=True)
                        for _ in range(2)]
    else:
        bucket = GradBucket(params, bind_grads=dist_on)
    if split_opt and not zero:
        side = torch.cuda.Stream(device=dev)
    pipe = {"k": 0, "done": [None, None]}
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    H_, W_ = args.height, args.width
    up_color = torch.randn(3, H_, W_, device=dev, generator=g)
    up_depth = torch.randn(1, H_, W_, device=dev, generator=g) * 0.1
    up_feat = torch.randn(args.features, H_, W_, device=dev, generator=g) if args.features else None

    # per-camera instance counts for the algorithmic byte model
    def instance_counts():
        """Per camera of the rank: list instances actually binned (the byte
        model's L), visible Gaussians and the reference's num_rendered, of
        the parameters as they are now."""
        res = []
        with torch.no_grad():
            rv = params2rendervar(params, label)
            from dynamic3dgaussians_amd import _C
            for s in settings:
                # one camera (and its tile window) through the batch entry point
                out = _C.rasterize_gaussians_batch(
                    s.bg, rv["means3D"], rv["colors_precomp"], rv.get("semantic_feature"),
                    rv["opacities"], rv["scales"], rv["rotations"], 1.0, torch.Tensor([]),
                    s.viewmatrix.reshape(1, 16), s.projmatrix.reshape(1, 16), [s.c_x], [s.c_y], [s.tanfovx],
                    [s.tanfovy], H_, W_, torch.Tensor([]), 0, s.campos.reshape(1, 3), False, False,
                    compat=args.compat, windows=[s.tile_window])
                res.append((int(out[9][0]), int((out[5][0] > 0).sum().item()), int(out[0][0])))
        return res

    # The parameters train during the run (Adam on fixed synthetic upstream
    # gradients), so the scene the kernels render drifts from step to step:
    # the counts are taken before the timed steps and again after them, and
    # the byte model uses their mean.  (--full: 27 forwards of their own)
    inst0 = instance_counts() if args.full else None

    # 4 = the box's hardware queues per process (GPU_MAX_HW_QUEUES): measured
    # 822 / 846 / 871 / 912 / 888 Mpix/s at 1 / 2 / 3 / 4 / 6 streams
    n_streams = max(1, int(os.environ.get("GS_BENCH_STREAMS", "4")))
    if hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
        # the leaves' accumulation crosses the camera streams by design
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(device=dev) for _ in range(n_streams - 1)]
    # the sync-free forward (gs_forward_batch; GS_BENCH_SYNC_FREE=0: the
    # two-phase plan -> host read -> render order of the reference)
    sync_free = os.environ.get("GS_BENCH_SYNC_FREE", "1") != "0"
    # the binning passes' walk in 3-D Morton order of the means
    # (GaussianRasterizerBatch(spatial_order=...), gs_gaussians.walk_order):
    # "auto" (default) once the lists outgrow the bucket pass's LDS staging
    walk = {"1": True, "0": False}.get(os.environ.get("GS_BENCH_WALK", "auto"), "auto")
    means2D_placeholder = torch.zeros_like(params["means3D"])

    # one upstream gradient per camera, materialized once (the batch's
    # backward reads [C, ...] images like C per-camera backwards do)
    def batch_inputs(setts, n_sub=1):
        n_sub = max(1, min(n_sub, len(setts), len(streams)))
        parts = []
        for gi in range(n_sub):
            idx = list(range(gi, len(setts), n_sub))
            C_ = len(idx)
            ups = (up_color.expand(C_, -1, -1, -1).contiguous(), up_depth.expand(C_, -1, -1, -1).contiguous(),
                   up_feat.expand(C_, -1, -1, -1).contiguous() if up_feat is not None else None)
            parts.append((GaussianRasterizerBatch([setts[i] for i in idx], raw_params=raw, sync_free=sync_free,
                                                  spatial_order=walk),
                          ups, streams[gi]))
        return parts

    batch_parts = batch_inputs(settings, args.sub_batches)

    # --dump-outputs: the rasterizer calls of the last timed step leave what
    # they returned here (one entry per call: a camera batch or one camera)
    last = {"on": False, "calls": []}

    def keep(im, radius, depth, feat=None):
        if last["on"]:
            last["calls"].append({"image": im, "radii": radius, "depth": depth, "feature": feat})

    def run_part(ras, ups, rv, ready=None, grad_into=None):
        up_c, up_d, up_f = ups
        if up_f is not None:  # G3 call (label + semantic_feature)
            im, radius, feat, depth, _ = ras(**rv, feature_ready=ready, grad_into=grad_into)
            torch.autograd.backward([im, depth, feat], [up_c, up_d, up_f])
            keep(im, radius, depth, feat)
        else:                 # G2 call (label only)
            im, radius, depth, _ = ras(**rv, grad_into=grad_into)
            torch.autograd.backward([im, depth], [up_c, up_d])
            keep(im, radius, depth)

    # the raw parameters' GaussianRasterizer argument names (raw_rendervar)
    arg_of = {"means3D": "means3D", "rgb_colors": "colors_precomp", "unnorm_rotations": "rotations",
              "logit_opacities": "opacities", "log_scales": "scales", "semantic_feature": "semantic_feature"}

    def step_zero(parts):
        """One rank's step with the sharded Adam (distributed.ShardedStep):
        the backward writes the gradients into the exchange buffers; geometry
        reduce-scatter + Adam on the rank's slice + all-gather in line; with
        `overlap` the feature exchange and update behind the next step's
        projection and binning (their blend waits on the event),
        double-buffered."""
        main = torch.cuda.current_stream(dev)
        zs.begin()
        rv = raw_rendervar(params, label, means2D_placeholder)
        if len(parts) == 1:
            run_part(parts[0][0], parts[0][1], rv, ready=zs.feature_ready, grad_into=zs.grad_into(arg_of))
        else:
            # sub-batches on their own streams accumulate through autograd
            zs.drain()
            zs.bind_grads()
            for _, _, st in parts:
                st.wait_stream(main)
            for ras, ups, st in parts:
                with torch.cuda.stream(st):
                    run_part(ras, ups, rv)
            for _, _, st in parts:
                main.wait_stream(st)
        zs.finish()

    def drain():
        """Overlap mode: the main stream waits for every pending feature update."""
        if zero:
            zs.drain()
        elif split_opt:
            for ev in pipe["done"]:
                if ev is not None:
                    torch.cuda.current_stream(dev).wait_event(ev)

    def step_overlap(parts):
        main = torch.cuda.current_stream(dev)
        k = pipe["k"]
        fb = feat_buckets[k % 2]
        if pipe["done"][k % 2] is not None:  # the exchange of step k-2 read this buffer
            main.wait_event(pipe["done"][k % 2])
        fb.bind()
        fb.zero_grad()
        bucket.zero_grad()
        rv = raw_rendervar(params, label, means2D_placeholder) if raw else params2rendervar(params, label)
        for ras, ups, _ in parts:
            run_part(ras, ups, rv, ready=pipe["done"][(k - 1) % 2])
        bucket.all_reduce()          # geometry: on the critical path, issued first
        work = fb.all_reduce_async()  # features: behind the next step
        opt.step()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if work is not None:
                work.wait()
            opt_feat.step()
            ev = torch.cuda.Event()
            ev.record(side)
        pipe["done"][k % 2] = ev
        pipe["k"] = k + 1

    def step_local_overlap(parts):
        """One rank: the geometry Adam on the main stream, the feature Adam on
        the side stream behind the next step's projection and binning."""
        main = torch.cuda.current_stream(dev)
        bucket.zero_grad()
        rv = raw_rendervar(params, label, means2D_placeholder) if raw else params2rendervar(params, label)
        for ras, ups, _ in parts:
            run_part(ras, ups, rv, ready=pipe["done"][0])
        opt.step()
        side.wait_stream(main)
        fg = params["semantic_feature"].grad
        with torch.cuda.stream(side):
            opt_feat.step()
            ev = torch.cuda.Event()
            ev.record(side)
        if fg is not None:  # read on the side stream after the main stream drops it
            fg.record_stream(side)
        pipe["done"][0] = ev
        pipe["k"] += 1

    def step_batch(parts=batch_parts):
        if zero:
            return step_zero(parts)
        if overlap and len(parts) == 1:
            return step_overlap(parts)
        if local_overlap and len(parts) == 1:
            return step_local_overlap(parts)
        drain()
        if overlap:
            feat_buckets[0].bind()
            feat_buckets[0].zero_grad()
        bucket.zero_grad()
        rv = raw_rendervar(params, label, means2D_placeholder) if raw else params2rendervar(params, label)
        if len(parts) == 1:
            run_part(parts[0][0], parts[0][1], rv)
        else:
            # sub-batches on their own streams: autograd keeps each one's
            # backward on its forward's stream and orders the leaves'
            # gradient accumulation across them
            main = torch.cuda.current_stream(dev)
            for _, _, st in parts:
                st.wait_stream(main)
            for ras, ups, st in parts:
                with torch.cuda.stream(st):
                    run_part(ras, ups, rv)
            for _, _, st in parts:
                main.wait_stream(st)
        bucket.all_reduce()
        opt.step()
        if overlap:
            feat_buckets[0].all_reduce()
        if split_opt:
            opt_feat.step()

    def step_single_camera():
        """The per-camera drop-in with one camera: the reference's training
        iteration as train.py writes it (params2rendervar's activations in
        torch, GaussianRasterizer, one backward, the optimizer step)."""
        drain()
        if zero:
            zs.bind_grads()
        else:
            if overlap:
                feat_buckets[0].bind()
                feat_buckets[0].zero_grad()
            bucket.zero_grad()
        rv = params2rendervar(params, label)
        ras = GaussianRasterizer(settings[0])
        if up_feat is not None:
            im, radius, feat, depth, _ = ras(**rv)
            torch.autograd.backward([im, depth, feat], [up_color, up_depth, up_feat])
            keep(im, radius, depth, feat)
        else:
            im, radius, depth, _ = ras(**rv)
            torch.autograd.backward([im, depth], [up_color, up_depth])
            keep(im, radius, depth)
        if zero:
            zs.finish(inline=True)
            return
        bucket.all_reduce()
        opt.step()
        if overlap:
            feat_buckets[0].all_reduce()
        if split_opt:
            opt_feat.step()

    def step(mode=args.mode):
        if mode == "batch":
            return step_batch()
        if len(settings) == 1:
            return step_single_camera()
        drain()
        if zero:
            zs.bind_grads()
        else:
            if overlap:
                feat_buckets[0].bind()
                feat_buckets[0].zero_grad()
            bucket.zero_grad()
        if sink is not None:
            sink.reset()
        rv = params2rendervar(params, label)
        # The activations are shared by all cameras of the step: render from
        # detached leaves, let autograd sum the per-camera gradients on them,
        # then run the activation backward once (same gradients as
        # back-propagating every camera through the activations).
        leaves = {k: v.detach().requires_grad_(True) for k, v in rv.items()
                  if isinstance(v, torch.Tensor) and v.requires_grad}
        rvl = dict(rv, **leaves)
        # Cameras alternate over `n_streams` HIP streams: one camera's small
        # latency-bound kernels (preprocess, binning) and its host round trip
        # (the plan's num_rendered read) overlap another camera's blend
        # kernels.  Autograd runs each camera's backward on its forward's
        # stream and orders the gradient accumulation across streams.
        main = torch.cuda.current_stream(dev)
        for st in streams:
            st.wait_stream(main)
        for i, s in enumerate(settings):
            with torch.cuda.stream(streams[i % len(streams)]):
                ras = GaussianRasterizer(s)
                if up_feat is not None:  # G3 call (label + semantic_feature)
                    im, radius, feat, depth, _ = ras(**rvl)
                else:                    # G2 call (label only)
                    im, radius, depth, _ = ras(**rvl)
                outs, grads = [im, depth], [up_color, up_depth]
                if up_feat is not None:
                    outs.append(feat)
                    grads.append(up_feat)
                torch.autograd.backward(outs, grads)
                keep(im, radius, depth, feat if up_feat is not None else None)
        for st in streams:
            main.wait_stream(st)
        summed = sink.gradients() if sink is not None else {k: v.grad for k, v in leaves.items()}
        keys = [k for k in leaves if k != "means2D" and summed.get(k) is not None]
        torch.autograd.backward([rv[k] for k in keys], [summed[k] for k in keys])
        if zero:
            zs.finish(inline=True)
            return
        bucket.all_reduce()
        opt.step()
        if overlap:
            feat_buckets[0].all_reduce()
        if split_opt:
            opt_feat.step()

    for _ in range(args.warmup):
        step()
    # one untimed step with every stage timed: the per-stage breakdown and the
    # dominant kernel; the timed region then records events around that kernel
    # only (each timed stage costs an event pair on the stream).  The stage
    # timing is --full's; the step itself runs in a plain run too, without
    # events in it or in the timed steps, so the timed steps are the same
    # optimizer steps W + 2 .. W + 1 + K with and without --full (and leave
    # the same parameters).
    torch.cuda.synchronize()
    if args.full:
        _lib.timing_enable(True)
    step()
    if args.full:
        all_stages = _lib.timing_read()
        _lib.timing_enable(False)
        stage_ms = {k: v[0] for k, v in all_stages.items()}
        dom = max(stage_ms, key=stage_ms.get)
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    if args.full:
        _lib.timing_enable(True, stages=[dom])

    def plan_counts():
        """(forward calls, capacity retries) of the camera batch's sync-free plans."""
        pl = [p_[0].plan for p_ in batch_parts if p_[0].plan is not None] if args.mode == "batch" else []
        return sum(p_.calls for p_ in pl), sum(p_.retries for p_ in pl)
    plan0 = plan_counts()
    t0 = time.perf_counter()
    host_marks = []
    for _ in range(args.steps):
        step()
        host_marks.append(time.perf_counter())
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    plan1 = plan_counts()
    if args.full:
        stages = _lib.timing_read()
        _lib.timing_enable(False)
    drain()
    if args.full:
        inst1 = instance_counts()
        inst = [tuple((a + b) / 2 for a, b in zip(x, y)) for x, y in zip(inst0, inst1)]
    if args.dump_params and rank == 0:
        drain()
        torch.cuda.synchronize()
        np.savez(args.dump_params, **{k: v.detach().cpu().numpy() for k, v in params.items()})
    if dist_on:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # the other call pattern on the same scene, timed the same way (reported
    # beside the headline: the per-camera drop-in or the camera batch)
    other = other_mode(args.mode, my_windows is not None, strong, world,
                       args.full and os.environ.get("GS_BENCH_OTHER") != "0")
    for _ in range(args.warmup if other else 0):
        step(other)
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    t1 = time.perf_counter()
    for _ in range(args.steps if other else 0):
        step(other)
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    other_elapsed = time.perf_counter() - t1
    if dist_on:
        t = torch.tensor([other_elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        other_elapsed = float(t.item())

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        ta = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - ta
        if dist_on:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    # The north star's 27-camera step split over the ranks (configs[3], strong
    # scaling), measured after a weak-scaling headline at N > 1; at N = 1 it
    # is the headline's own step (27 cameras on one rank).
    split = None
    sharding_note = ("first N*(T//N) cameras whole, c mod N; the T%N left over cut into bands of tile rows "
                     "balancing the ranks' tile-list instances (distributed.shard_camera_windows)"
                     if args.split == "windows" else
                     "camera c on rank c mod N (distributed.shard_cameras)")
    if args.full and not strong and args.mode == "batch":
        n_split = args.cams
        if world > 1:
            rig_s = camera_rig(n_split, args.width, args.height, seed=args.seed)
            costs_s = rig_costs(rig_s, params0, label, args, dev) if args.split == "windows" else None
            ws_s = None
            if args.split == "windows" and args.balance == "measured":
                ws_s, _ = measured_balance(n_split, world, rank, rig_s, params0, label, args, dev, costs_s)
            mine = split_shard(n_split, rank, world, args.split, args.width, args.height, costs_s, ws_s)
            wins = [w for _, w in mine] if any(w is not None for _, w in mine) else None
            parts_s = batch_inputs(make_settings([rig_s[c] for c, _ in mine], dev, args.compat, None, wins),
                                   args.sub_batches)
            el_s = timed(lambda: step_batch(parts_s))
            cams_rank = [len(split_shard(n_split, r, world, args.split, args.width, args.height, costs_s, ws_s))
                         for r in range(world)]
            del parts_s
        else:
            el_s, cams_rank = elapsed, [args.cams]
        ms_s = el_s / args.steps * 1e3
        split = {"cams_total": n_split, "cams_per_rank": cams_rank, "ms_per_step": round(ms_s, 3),
                 "value": round(n_split * W_ * H_ / 1e6 / (ms_s / 1e3), 3), "unit": "Mpix/s",
                 "scaling": "strong", "sharding": sharding_note}

    # --dump-outputs: the parameters the timed steps leave differ from run to
    # run (the backward's float atomics sum in another order every run, and
    # the Adam steps on fixed upstream gradients amplify that), so the step
    # that is written is one more step of the timed path, untimed, from the
    # seeded parameters the run started with: the same inputs every run and in
    # every build.  Every rank takes it (its collectives); rank 0 writes.
    if args.dump_outputs:
        drain()
        torch.cuda.synchronize()  # every stream of the earlier steps is done with the parameters
        with torch.no_grad():
            for k_, v_ in params.items():
                v_.copy_(params0[k_])
        torch.cuda.synchronize()
        last["on"] = True
        step()
        last["on"] = False
        drain()
        torch.cuda.synchronize()
        if rank == 0:
            dump_outputs(args.dump_outputs, last["calls"], params, args.seed)
        last["calls"] = []

    ms_per_step = elapsed / args.steps * 1e3
    n_cams_total = args.cams_total if strong else world * args.cams
    mpix_total = n_cams_total * W_ * H_ / 1e6
    if args.proxy_world:
        # one rank's share: its own windows' pixels
        gx, gy = (W_ + 15) // 16, (H_ + 15) // 16
        share = sum(1.0 if w is None else (w[2] - w[0]) * (w[3] - w[1]) / (gx * gy)
                    for w in (my_windows or [None] * len(my_cams)))
        mpix_total = share * W_ * H_ / 1e6
    value = mpix_total / (ms_per_step / 1e3)

    roofline = None
    if args.full:
        # roofline of the dominant stage (live HIP-event durations over the timed region)
        cams_per_launch = len(batch_parts[0][0].settings_list) if args.mode == "batch" else 1
        per_cam_bytes = [stage_bytes(L, Pv, args.gaussians, W_, H_, args.features, args.compat, cams_per_launch)
                         for L, Pv, _ in inst]
        launches = stages[dom][1]
        alg_bytes_total = sum(b[dom] for b in per_cam_bytes) * args.steps
        avg_ms = stages[dom][0] / max(launches, 1)
        alg_per_launch = alg_bytes_total / max(launches, 1)
        achieved = alg_per_launch / (avg_ms / 1e3) / 1e9 if avg_ms > 0 else 0.0
        # the PMC-derived views only for the workload the counters were measured on
        workload = {"gaussians": args.gaussians, "width": W_, "height": H_, "features": args.features,
                    "compat": args.compat, "rig": len(rig), "cams_per_launch": cams_per_launch, "seed": args.seed}
        pmc = pmc_for(workload) if args.mode == "batch" and world == 1 else {}
        meas = (pmc.get("traffic") or {}).get("bytes_per_camera", {})
        hbm = {"achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(achieved / HBM_PEAK_GBS, 4),
               "traffic": int(meas[dom] * cams_per_launch) if dom in meas else None}
        issue = issue_view(pmc, dom, avg_ms, cams_per_launch)
        atomics = atomic_view(pmc, dom, avg_ms, cams_per_launch)
        # the binding roof: the highest of the HBM (algorithmic bytes), float-atomic
        # and issue fractions of the dominant kernel
        roofs = {"hbm": hbm}
        if atomics:
            roofs["atomics"] = atomics
        if issue:
            roofs["issue"] = issue
        bound = max(roofs, key=lambda r: roofs[r]["frac"])
        b = roofs[bound]
        if bound == "issue":
            b = {"achieved": b["frac"], "peak": 1.0, "unit": "fraction of SIMD issue cycles", "frac": b["frac"]}
        roofline = {"bound": bound, "achieved": b["achieved"], "peak": b["peak"], "unit": b["unit"], "frac": b["frac"],
                    "traffic": hbm["traffic"], "kernel": dom, "avg_launch_ms": round(avg_ms, 4),
                    "alg_bytes_per_launch": int(alg_per_launch), "cams_per_launch": cams_per_launch,
                    "hbm": hbm, "atomics": atomics, "issue": issue,
                    "pmc_workload_matched": bool(pmc),
                    "stages": stage_table(stage_ms, {k: np.mean([pb[k] for pb in per_cam_bytes])
                                                     for k in per_cam_bytes[0]}, pmc,
                                          len(my_cams))}

    result = {
        "metric": METRIC, "value": round(value, 3), "unit": "Mpix/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
        "dtype": "f32",
        "dtype_note": ("fp32 blend on the vector ALUs; the feature blend and the backward's per-Gaussian "
                       "sums as matrix-core contractions of split operands with fp32 accumulation -- the "
                       "weights w = alpha T and their partners as fp16 two-piece splits under power-of-two "
                       "scales (products to ~3 x 2^-24 relative), the geometry weights as 3-piece bf16 "
                       "splits (2^-26): tests/test_gpu_parity.py and test_gpu_envelope.py hold them to the "
                       "oracle at 1e-5 / 1e-4 and within 10x its fp32 summation-order spread"),
        "data": "synthetic",
        "config": {"workload": (f"rank {args.proxy_rank} of {args.proxy_world} of {args.gaussians // 1000}k "
                                f"Gaussians x {args.cams_total} cams split ({args.split})" if args.proxy_world else
                                f"{args.gaussians // 1000}k Gaussians x {args.cams_total} cams split over "
                                f"{world} rank(s) ({args.split})" if strong else
                                f"{args.gaussians // 1000}k Gaussians x {args.cams} cams/rank") +
                               f" x {W_}x{H_}, F={args.features} semantic channels, colors_precomp; "
                               "fwd+bwd of every camera + grad all-reduce + Adam",
                   "mode": ("camera batch (GaussianRasterizerBatch: one launch per stage for the rank's "
                            "cameras)" if args.mode == "batch" else "per camera (GaussianRasterizer drop-in)"),
                   "optimizer": (f"sharded Adam (ZeRO-1, distributed.ShardedStep): rank {z_rank}'s 1/{z_world} "
                                 "of the parameters, gradients written into the exchange buffer" if zero
                                 else optim_kind),
                   "streams": n_streams if args.mode == "percam" else len(batch_parts),
                   "forward": ("sync-free (gs_forward_batch: binning sized from the previous step)" if sync_free
                               and args.mode == "batch" else "two-phase (plan, host read, render)"),
                   # the timed window's sync-free forwards and how many re-rendered with exact lengths
                   # (0: every camera rendered once per step)
                   "sync_free_calls_timed": plan1[0] - plan0[0],
                   "sync_free_retries_timed": plan1[1] - plan0[1],
                   "binning_walk": ("3-D Morton order of the means (gs_gaussians.walk_order)"
                                    if args.mode == "batch" and any(p_[0]._walk is not None for p_ in batch_parts)
                                    else "id order"),
                   "activations": ("in-kernel (raw parameters, GS_FLAG_ACTIVATE)" if raw and args.mode == "batch"
                                   else "torch ops (params2rendervar)"),
                   "grad_sum": ("in-kernel (camera sum in preprocess_bwd)" if args.mode == "batch" else
                                "in-kernel (GradientSink)" if use_sink else
                                "none (one camera: the reference's train.py iteration)" if len(my_cams) == 1 else
                                "autograd"),
                   "gaussians": args.gaussians, "cams_per_rank": len(my_cams), "width": W_,
                   "height": H_, "feature_channels": args.features, "compat": args.compat,
                   "parallelism": f"camera-sharded dp{world}",
                   "grad_exchange": ("geometry reduce-scatter + sharded Adam + all-gather in line; the features' "
                                     "behind the next step's projection and binning" if (zero and overlap) else
                                     "reduce-scatter + sharded Adam + all-gather" if (zero and world > 1) else
                                     f"none (a one-GPU stand-in for rank {z_rank} of {z_world}: its Adam slice, "
                                     "no collective)" if (zero and args.proxy_world) else
                                     "reduce-scatter + sharded Adam + all-gather (forced at one rank)" if zero else
                                     "geometry all-reduce before Adam; feature all-reduce + Adam overlapped with the "
                                     "next step's projection and binning" if overlap else
                                     "one all-reduce before Adam" if world > 1 else
                                     "none (one rank); the feature Adam step overlapped with the next step's "
                                     "projection and binning" if local_overlap else "none (one rank)")},
        "full": args.full,
    }
    if args.full:
        result.update({
            "roofline": roofline,
            "stages_ms_per_step": {k: round(v, 4) for k, v in stage_ms.items()},
            "split_step": split,
            "other_mode": None if other is None else {
                "mode": other, "ms_per_step": round(other_elapsed / args.steps * 1e3, 3),
                "value": round(mpix_total / (other_elapsed / args.steps), 3),
                "streams": n_streams if other == "percam" else 1},
            "instances_per_cam": int(np.mean([L for L, _, _ in inst])),
            "instances_per_cam_before_after": [int(np.mean([x[0] for x in inst0])),
                                               int(np.mean([x[0] for x in inst1]))],
            "num_rendered_per_cam": int(np.mean([R for _, _, R in inst])),
        })
    if args.dump_outputs:
        result["outputs_dir"] = args.dump_outputs
    if strong:
        # the split's work model: every rank's pieces and modelled load
        # (row_cost instances + PIECE_FRACTION x a mean camera per piece)
        s_world = args.proxy_world if args.proxy_world else world
        gx_, gy_ = (W_ + 15) // 16, (H_ + 15) // 16
        model = []
        rc_, pc_ = costs if costs is not None else (None, 0.0)
        for r_ in range(s_world):
            sh_ = split_shard(args.cams_total, r_, s_world, args.split, W_, H_, costs, wscale)
            load = 0.0
            for c_, w_ in sh_:
                rows = range(gy_) if w_ is None else range(w_[1], w_[3])
                load += (sum(rc_[c_][y] for y in rows) + pc_) if rc_ is not None else 0.0
            model.append({"rank": r_, "pieces": len(sh_), "model_load": round(load, 1),
                          "shard": [[c_, w_] for c_, w_ in sh_]})
        result["split_model"] = {"piece_fraction": PIECE_FRACTION, "piece_cost": round(pc_, 2),
                                 "balance": args.balance,
                                 "whole_scale": [round(x, 4) for x in wscale] if wscale else None,
                                 "cut_fwd_bwd_ms": [[round(x, 4) for x in r] for r in first_ms] if first_ms else None,
                                 "row_cost": [[int(v) for v in r] for r in rc_] if rc_ else None,
                                 "ranks": model}
    if args.step_times:
        result["host_step_ms"] = [round((b - a) * 1e3, 3) for a, b in zip([t0] + host_marks, host_marks)]
        result["tail_ms"] = round((t0 + elapsed - host_marks[-1]) * 1e3, 3) if world == 1 else None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and settings[0].tile_window is None:
        cb, psnr, psnr_gt = cpu_baseline(args, params0, label, my_cams[0], settings[0], dev)
        result["cpu_baseline"] = cb
        result["psnr_vs_oracle_db"] = round(psnr, 2) if np.isfinite(psnr) else "inf"
        result["psnr_vs_gt_db"] = psnr_gt
    if rank == 0:
        sys.stdout.flush()
        os.write(line_fd, (json.dumps(result) + "\n").encode())
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
