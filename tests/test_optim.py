"""Fused Adam + densification statistics against
torch.optim.Adam and the reference's statistics code, on the reference's
parameter groups (train.py:119-135: per-group lr, two of them 0, eps=1e-15).

Adam: the kernel evaluates torch's multi-tensor Adam op sequence in fp32
(lerp, mul, addcmul, sqrt, div, add, addcdiv; scalars rounded once from
double like torch's scalar arguments; the multiply-adds torch's ROCm build
contracts as explicit fmas), so parameters and moments are BIT-IDENTICAL to
torch.optim.Adam's (tools/adam_probe.py reports the per-word agreement)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LRS = {"means3D": 0.0000016 * 3.2, "rgb_colors": 0.000025, "seg_colors": 0.0, "unnorm_rotations": 0.0,
       "logit_opacities": 0.05, "log_scales": 0.001, "cam_m": 1e-5, "cam_c": 1e-5}
SHAPES = {"means3D": 3, "rgb_colors": 3, "seg_colors": 3, "unnorm_rotations": 4, "logit_opacities": 1,
          "log_scales": 3}


def make_params(P=10007, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    params = {k: torch.randn(P, c, device="cuda", generator=g) for k, c in SHAPES.items()}
    params["cam_m"] = torch.randn(27, 3, device="cuda", generator=g)
    params["cam_c"] = torch.randn(27, 3, device="cuda", generator=g)
    return {k: torch.nn.Parameter(v.contiguous()) for k, v in params.items()}


def make_opt(cls, params, **kw):
    groups = [{"params": [v], "name": k, "lr": LRS[k]} for k, v in params.items()]
    return cls(groups, lr=0.0, eps=1e-15, **kw)


def set_grads(params, step, skip=()):
    g = torch.Generator(device="cuda").manual_seed(100 + step)
    for k, p in params.items():
        p.grad = None if k in skip else torch.randn(p.shape, device="cuda", generator=g) * 10 ** (step % 3 - 1)


def assert_params_equal(a, b):
    for k in a:
        x, y = a[k].detach(), b[k].detach()
        assert torch.equal(x, y), (k, (x - y).abs().max().item(), (x != y).float().mean().item())


def _clone(params):
    return {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}


def test_fused_adam_matches_torch_adam():
    from dynamic3dgaussians_amd.optim import FusedAdam
    ref = make_params()
    ours = _clone(ref)
    o_ref = make_opt(torch.optim.Adam, ref)
    o_ours = make_opt(FusedAdam, ours)
    for step in range(6):
        skip = ("cam_m",) if step == 2 else ()
        set_grads(ref, step, skip)
        set_grads(ours, step, skip)
        o_ref.step()
        o_ours.step()
        assert_params_equal(ours, ref)
    for k in ref:
        sr, so = o_ref.state[ref[k]], o_ours.state[ours[k]]
        assert sr["step"].item() == so["step"].item(), k
        assert so["step"].device.type == "cpu" and so["step"].dtype == torch.float32
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(so[key], sr[key]), (k, key)
    # lr 0 groups never move, but their moments do (like torch)
    assert torch.equal(ours["seg_colors"].detach(), ref["seg_colors"].detach())


def _cat_params(new_params, params, optimizer):
    """The reference's cat_params_to_optimizer (external.py:158-182), restated."""
    for k, v in new_params.items():
        group = [g for g in optimizer.param_groups if g["name"] == k][0]
        st = optimizer.state.get(group["params"][0], None)
        st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(v)), dim=0)
        st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(v)), dim=0)
        del optimizer.state[group["params"][0]]
        group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], v), dim=0).requires_grad_(True))
        optimizer.state[group["params"][0]] = st
        params[k] = group["params"][0]
    return params


def _remove(to_keep, params, optimizer):
    """The reference's remove_points (external.py:185-207), restated."""
    for k in list(params):
        if k in ("cam_m", "cam_c"):
            continue
        group = [g for g in optimizer.param_groups if g["name"] == k][0]
        st = optimizer.state.get(group["params"][0], None)
        st["exp_avg"] = st["exp_avg"][to_keep]
        st["exp_avg_sq"] = st["exp_avg_sq"][to_keep]
        del optimizer.state[group["params"][0]]
        group["params"][0] = torch.nn.Parameter(group["params"][0][to_keep].requires_grad_(True))
        optimizer.state[group["params"][0]] = st
        params[k] = group["params"][0]
    return params


def test_fused_adam_survives_reference_state_surgery():
    from dynamic3dgaussians_amd.optim import FusedAdam
    ref = make_params(P=5000, seed=1)
    ours = _clone(ref)
    o_ref, o_ours = make_opt(torch.optim.Adam, ref), make_opt(FusedAdam, ours)
    for step in range(2):
        set_grads(ref, step)
        set_grads(ours, step)
        o_ref.step()
        o_ours.step()
    sel = torch.arange(0, 5000, 7, device="cuda")
    for params, opt in ((ref, o_ref), (ours, o_ours)):
        new = {k: v.detach()[sel] for k, v in params.items() if k not in ("cam_m", "cam_c")}
        _cat_params(new, params, opt)
        keep = torch.ones(params["means3D"].shape[0], dtype=torch.bool, device="cuda")
        keep[::5] = False
        _remove(keep, params, opt)
    for step in range(2, 5):
        set_grads(ref, step)
        set_grads(ours, step)
        o_ref.step()
        o_ours.step()
    assert_params_equal(ours, ref)


def _ref_stats(variables, radius):
    """train.py:288-290 + external.py:136-140."""
    seen = radius > 0
    variables["max_2D_radius"][seen] = torch.max(radius[seen], variables["max_2D_radius"][seen])
    variables["means2D_gradient_accum"][seen] += torch.norm(variables["means2D"].grad[seen, :2], dim=-1)
    variables["denom"][seen] += 1
    variables["seen"] = seen


def _stats_vars(P, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    m2.grad = torch.randn(P, 3, device="cuda", generator=g) * 1e-3
    return {"max_2D_radius": torch.rand(P, device="cuda", generator=g) * 20,
            "means2D_gradient_accum": torch.rand(P, device="cuda", generator=g),
            "denom": torch.randint(0, 9, (P,), device="cuda", generator=g).float(),
            "means2D": m2}


def test_densify_stats_match_reference():
    from dynamic3dgaussians_amd.optim import densify_stats
    P = 30001
    g = torch.Generator(device="cuda").manual_seed(4)
    radius = (torch.randint(-3, 40, (P,), device="cuda", generator=g)).clamp_min(0).int()
    a, b = _stats_vars(P, 5), _stats_vars(P, 5)
    _ref_stats(a, radius)
    densify_stats(b, radius)
    assert torch.equal(b["max_2D_radius"], a["max_2D_radius"])
    assert torch.equal(b["denom"], a["denom"])
    assert torch.equal(b["means2D_gradient_accum"], a["means2D_gradient_accum"])
    assert torch.equal(b["seen"], a["seen"])
    # max radius only (the non-densifying timesteps)
    c = _stats_vars(P, 5)
    acc0 = c["means2D_gradient_accum"].clone()
    densify_stats(c, radius, accumulate=False)
    assert torch.equal(c["max_2D_radius"], a["max_2D_radius"])
    assert torch.equal(c["means2D_gradient_accum"], acc0)


def test_step_with_fused_stats_equals_separate():
    from dynamic3dgaussians_amd.optim import FusedAdam, densify_stats
    P = 10007
    base = make_params(P=P, seed=2)
    p1, p2 = _clone(base), _clone(base)
    o1, o2 = make_opt(FusedAdam, p1), make_opt(FusedAdam, p2)
    g = torch.Generator(device="cuda").manual_seed(8)
    radius = torch.randint(0, 30, (P,), device="cuda", generator=g).int()
    v1, v2 = _stats_vars(P, 9), _stats_vars(P, 9)
    set_grads(p1, 0)
    set_grads(p2, 0)
    densify_stats(v1, radius)
    o1.step()
    o2.step(stats=(v2, radius))
    for k in p1:
        assert torch.equal(p1[k].detach(), p2[k].detach()), k
    for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "seen"):
        assert torch.equal(v1[k], v2[k]), k


def test_fused_adam_step_counts_follow_external_changes():
    """FusedAdam caches each parameter's step count against its state tensor;
    a step tensor replaced (load_state_dict, state surgery) or changed in place
    from outside must be re-read, exactly as torch.optim.Adam reads it."""
    from dynamic3dgaussians_amd.optim import FusedAdam
    ref = make_params(P=4099, seed=3)
    ours = _clone(ref)
    o_ref = make_opt(torch.optim.Adam, ref)
    o_ours = make_opt(FusedAdam, ours)

    def both_step(step):
        set_grads(ref, step)
        set_grads(ours, step)
        o_ref.step()
        o_ours.step()

    for step in range(3):
        both_step(step)
    for o, ps in ((o_ref, ref), (o_ours, ours)):
        o.state[ps["means3D"]]["step"] = torch.tensor(40.0)   # replaced tensor
        o.state[ps["log_scales"]]["step"].fill_(7.0)           # changed in place
    both_step(3)
    for o, ps in ((o_ref, ref), (o_ours, ours)):
        assert float(o.state[ps["means3D"]]["step"]) == 41.0
        assert float(o.state[ps["log_scales"]]["step"]) == 8.0
    # a state_dict round trip (new step tensors) mid-training
    o_ours.load_state_dict(o_ours.state_dict())
    for step in range(4, 6):
        both_step(step)
    assert_params_equal(ref, ours)
    for k in ref:
        assert float(o_ours.state[ours[k]]["step"]) == float(o_ref.state[ref[k]]["step"])


# ---- the branches of adam_stats_kernel / FusedAdam.step the tests above do
# not reach: the scalar path (a pointer off 16 bytes), chunk edges, more than
# MAX_TENSORS tensors, groups with their own betas / eps, empty tensors

DEV = "cuda"
# below a float4 (1, 3) | a chunk less one | a full chunk, no tail | a one-element tail | two full chunks
EDGE_NUMELS = (1, 3, 4095, 4096, 4097, 8192)


def _offset_view(t):
    """The same values one float into a larger buffer: 4-byte aligned, not 16."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _edge_values(seed, steps=3):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=g) for n in EDGE_NUMELS]
    grads = [[torch.randn(n, generator=g) * 10.0 ** (s - 1) for n in EDGE_NUMELS] for s in range(steps)]
    return p0, grads


def _run_edges(cls, p0, grads, layout, lr=1e-2, betas=(0.9, 0.999), eps=1e-15):
    """`steps` Adam steps over the EDGE_NUMELS tensors -> [(param, exp_avg,
    exp_avg_sq)] on the CPU.  layout: 'aligned', 'param' (parameters are
    offset views) or 'grad' (gradients are offset views)."""
    place = lambda t, off: _offset_view(t.to(DEV)) if off else t.to(DEV).clone()  # noqa: E731
    params = [torch.nn.Parameter(place(t, layout == "param")) for t in p0]
    opt = cls([{"params": [p], "lr": lr * (k + 1)} for k, p in enumerate(params)], lr=0.0, betas=betas, eps=eps)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = place(g, layout == "grad")
            assert (p.data_ptr() % 16 == 4) == (layout == "param")
            assert (p.grad.data_ptr() % 16 == 4) == (layout == "grad")
        opt.step()
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in params]


@pytest.mark.parametrize("layout", ["aligned", "param", "grad"])
def test_fused_adam_misaligned_storage_and_chunk_edges(layout):
    """vec == false (a parameter or a gradient one float off a 16-byte
    boundary) and numel around the 4096-element chunk, beside aligned twins:
    bit-identical to torch.optim.Adam on aligned storage."""
    from dynamic3dgaussians_amd.optim import FusedAdam
    p0, grads = _edge_values(21)
    ref = _run_edges(torch.optim.Adam, p0, grads, "aligned")
    ours = _run_edges(FusedAdam, p0, grads, layout)
    for n, a, b in zip(EDGE_NUMELS, ours, ref):
        for what, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
            assert torch.equal(x, y), (layout, n, what, (x - y).abs().max().item())


def _adam_float64(p0, grads, lrs, betas, eps):
    """Adam in float64 (Kingma & Ba, bias-corrected as torch does), numpy."""
    out = []
    for k, p in enumerate(p0):
        p = p.double().numpy().copy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        for t, gs in enumerate(grads, 1):
            g = gs[k].double().numpy()
            m = betas[0] * m + (1 - betas[0]) * g
            v = betas[1] * v + (1 - betas[1]) * g * g
            p = p - lrs[k] / (1 - betas[0] ** t) * m / (np.sqrt(v) / np.sqrt(1 - betas[1] ** t) + eps)
        out.append(p)
    return out


@pytest.mark.parametrize("layout", ["aligned", "param", "grad"])
def test_fused_adam_no_further_from_float64_than_torch(layout):
    """Three steps against a float64 Adam: per tensor, the fused result's
    max-abs error is at most twice that of torch.optim.Adam's fp32 result."""
    from dynamic3dgaussians_amd.optim import FusedAdam
    betas, eps, lr = (0.8, 0.99), 1e-8, 1e-2
    p0, grads = _edge_values(22)
    want = _adam_float64(p0, grads, [lr * (k + 1) for k in range(len(p0))], betas, eps)
    ref = _run_edges(torch.optim.Adam, p0, grads, "aligned", lr, betas, eps)
    ours = _run_edges(FusedAdam, p0, grads, layout, lr, betas, eps)
    for n, a, b, w in zip(EDGE_NUMELS, ours, ref, want):
        e_ours = np.abs(a[0].double().numpy() - w).max()
        e_torch = np.abs(b[0].double().numpy() - w).max()
        assert e_torch <= 1e-5  # the float64 restatement is the same Adam (updates are ~lr per step)
        assert e_ours <= 2 * e_torch, (layout, n, e_ours, e_torch)


def test_fused_adam_19_tensors_two_launches_stats_once():
    """19 tensors: launches of 16 and 3 (MAX_TENSORS); the statistics ride on
    the first launch only -- denom moves by exactly one where seen."""
    from dynamic3dgaussians_amd.optim import MAX_TENSORS, FusedAdam
    n_t, P = 19, 1000
    assert n_t > MAX_TENSORS
    g = torch.Generator().manual_seed(31)
    p0 = [torch.randn(100 + 37 * k, generator=g) for k in range(n_t)]
    radius = torch.randint(-2, 30, (P,), generator=g).clamp_min(0).int().to(DEV)
    assert 0 < int((radius > 0).sum()) < P
    results = []
    for cls in (torch.optim.Adam, FusedAdam):
        params = [torch.nn.Parameter(t.to(DEV).clone()) for t in p0]
        opt = cls([{"params": [p], "lr": 1e-3 * (k + 1)} for k, p in enumerate(params)], lr=0.0, eps=1e-15)
        v = _stats_vars(P, 32)
        denom0 = v["denom"].clone()
        for step in range(2):
            gg = torch.Generator().manual_seed(40 + step)
            for p in params:
                p.grad = torch.randn(p.shape, generator=gg).to(DEV)
            if cls is FusedAdam:
                opt.step(stats=(v, radius))
            else:
                _ref_stats(v, radius)
                opt.step()
        assert torch.equal(v["denom"], denom0 + 2.0 * (radius > 0))  # once per step
        results.append((params, opt, v))
    (pr, o_r, vr), (po, o_o, vo) = results
    for k in range(n_t):
        assert torch.equal(po[k].detach(), pr[k].detach()), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o_o.state[po[k]][key], o_r.state[pr[k]][key]), (k, key)
    for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "seen"):
        assert torch.equal(vo[k], vr[k]), k


def test_fused_adam_groups_with_own_betas_eps_empty_and_gradless():
    """Three groups with different betas / eps in one optimizer (one launch per
    hyper-parameter set), one tensor with numel == 0 and one without a
    gradient: as torch.optim.Adam."""
    from dynamic3dgaussians_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(51)
    shapes = {"a0": (4097,), "a1": (33, 3), "b0": (500, 4), "b_empty": (0, 3), "c0": (257,), "c_nograd": (64,)}
    p0 = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    hyper = {"a": dict(betas=(0.9, 0.999), eps=1e-15, lr=1e-3), "b": dict(betas=(0.8, 0.99), eps=1e-8, lr=2e-2),
             "c": dict(betas=(0.5, 0.9), eps=1e-3, lr=5e-3)}
    results = []
    for cls in (torch.optim.Adam, FusedAdam):
        params = {k: torch.nn.Parameter(t.to(DEV).clone()) for k, t in p0.items()}
        opt = cls([dict(params=[p for k, p in params.items() if k[0] == name], **h) for name, h in hyper.items()])
        for step in range(3):
            gg = torch.Generator().manual_seed(60 + step)
            for k, p in params.items():
                p.grad = None if k == "c_nograd" else torch.randn(p.shape, generator=gg).to(DEV)
            opt.step()
        results.append((params, opt))
    (pr, o_r), (po, o_o) = results
    for k in shapes:
        sr, so = o_r.state[pr[k]], o_o.state[po[k]]
        assert set(sr) == set(so), k  # no state without a gradient; state for the empty tensor
        if sr:
            assert float(sr["step"]) == float(so["step"]) == 3.0, k
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(so[key], sr[key]), (k, key, (so[key] - sr[key]).abs().max().item())
        assert torch.equal(po[k].detach(), pr[k].detach()), k
    assert torch.equal(po["c_nograd"].detach().cpu(), p0["c_nograd"])


@pytest.mark.parametrize("beta1", [0.6, 0.5, 0.3, 0.0])
def test_fused_adam_lerp_branch_of_small_beta1(beta1):
    """torch's lerp evaluates a + w (b - a) for a weight w = 1 - beta1 below 0.5
    and b - (b - a)(1 - w) from 0.5 up: beta1 = 0.5 is the first value on the
    second form, 0.3 one where its rounding differs from the first form's, 0.0
    the end (exp_avg = grad).  Moments and parameters stay bit-identical."""
    from dynamic3dgaussians_amd.optim import FusedAdam
    p0, grads = _edge_values(23)
    ref = _run_edges(torch.optim.Adam, p0, grads, "aligned", 1e-2, (beta1, 0.99), 1e-8)
    ours = _run_edges(FusedAdam, p0, grads, "aligned", 1e-2, (beta1, 0.99), 1e-8)
    for n, a, b in zip(EDGE_NUMELS, ours, ref):
        for what, x, y in zip(("exp_avg", "exp_avg_sq", "param"), a[1:] + a[:1], b[1:] + b[:1]):
            assert torch.equal(x, y), (beta1, n, what, (x - y).abs().max().item(), (x != y).float().mean().item())


@pytest.mark.parametrize("P", [1, 255, 256, 257])  # one thread | a block less one | a full block | one more
@pytest.mark.parametrize("visible", [False, True])
def test_densify_stats_block_edges_all_or_nothing(P, visible):
    """All radii <= 0: nothing changes and `seen` is all False; all radii > 0:
    every row is updated."""
    from dynamic3dgaussians_amd.optim import densify_stats
    g = torch.Generator().manual_seed(P)
    radius = torch.randint(1, 40, (P,), generator=g) if visible else torch.randint(-3, 1, (P,), generator=g)
    radius = radius.int().to(DEV)
    a, b = _stats_vars(P, 70 + P), _stats_vars(P, 70 + P)
    before = {k: b[k].clone() for k in ("max_2D_radius", "means2D_gradient_accum", "denom")}
    _ref_stats(a, radius)
    densify_stats(b, radius)
    for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "seen"):
        assert torch.equal(b[k], a[k]), k
    assert bool(b["seen"].all()) == visible and bool(b["seen"].any()) == visible
    if visible:
        assert torch.equal(b["denom"], before["denom"] + 1)
    else:
        for k, t in before.items():
            assert torch.equal(b[k], t), k
