"""The scene regularisers and the foreground gather (csrc/gs_scene_loss.hip) on the GPU against
regularizer_losses_torch in fp64 on the CPU, torch's own fp32 autograd on the device, and boolean
indexing.

Bounds: the losses within 2e-5 relative (the project's bar for the neighbour losses, DESIGN.md
9.2).  The gradients of the means, the colours and already-normalised rotations within 2.4e-7
relative L2: every element is +-g * (1 / N) or 0, which differs from the fp64 value by two fp32
roundings (the reciprocal, the product) of at most 2^-24 relative each, 1.2e-7 together; the
bar is two units in the last place, 2 * 2^-23.  The gradients of the raw-rotation
path within 1e-4 relative L2 (SURVEY.md 8(c)'s gradient bar).  The upstream gradients are fp32
values on both sides.

A workgroup takes 256 rows and the forward's grid is capped at 8 x 256 CUs = 2048 workgroups, so
the shapes are P = 1, 63, 64, 65 (around a wave), 257 (a second, partial workgroup) and
P = 2048 * 256 + 300 = 524588, where the grid-stride loop runs twice for the threads of the
first two workgroups and the last of those is partial; foreground fractions 0, 1 and about 0.4.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (_lib, foreground_split, gather_foreground, reference_extra_loss,
                                    regularizer_losses, regularizer_losses_torch)
from dynamic3dgaussians_amd.neighbor import neighbor_losses
from tests.test_neighbor import make_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_loss.npz")
LOSS_TOL, GRAD_TOL, RAW_GRAD_TOL = 2e-5, 2.4e-7, 1e-4
GRID_CAP = 8 * 256                  # workgroups: csrc/gs_scene_loss_layout.h SL_MAX_GROUPS
P_LOOPED = GRID_CAP * 256 + 300     # 524588
SIZES = (1, 63, 64, 65, 257, P_LOOPED)
FRACTIONS = (0.0, 1.0, 0.4)
UP = tuple(float(np.float32(u)) for u in (0.7, -1.3, 2.1))  # the upstream gradients, exact in fp32
TABLES = ("means3D", "rotations", "rgb_colors")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _case(P, frac):
    """fp32 CPU inputs, never modified: the three tables (rotations raw, of norm 0.5 .. 1.5), the
    mask and the reference's `variables`.  A tenth of the foreground heights, background
    coordinates and colours sit exactly on their kink."""
    gen = torch.Generator().manual_seed(1000 * P % 65521 + int(frac * 10))
    is_fg = torch.rand(P, generator=gen) < frac if 0.0 < frac < 1.0 else torch.full((P,), frac == 1.0)
    means = torch.randn(P, 3, generator=gen)
    raw = torch.nn.functional.normalize(torch.randn(P, 4, generator=gen)) * (0.5 + torch.rand(P, 1, generator=gen))
    col = torch.rand(P, 3, generator=gen)
    n_bg = int((~is_fg).sum())
    bg_pts = means[~is_fg] + 0.05 * torch.randn(n_bg, 3, generator=gen)
    unit = torch.nn.functional.normalize(raw[~is_fg])
    bg_rot = torch.nn.functional.normalize(unit + 0.05 * torch.randn(n_bg, 4, generator=gen))
    # The sign of q_hat - anchor is a decision.  On the raw path q_hat is computed, in fp32 by the
    # kernel and in fp64 by the reference, so an element within fp32's rounding of q_hat (6e-8) of
    # its anchor could take either sign (3 of the 2.1 M elements of the largest case would).  The
    # anchors keep 1e-5 away, a hundred roundings; the exact-zero kinks are in the other tables.
    bg_rot = torch.where((unit - bg_rot).abs() < 1e-5, unit - 1e-4, bg_rot)
    prev_col = col + 0.05 * torch.randn(P, 3, generator=gen)
    kink = torch.rand(P, generator=gen) < 0.1
    means[kink & is_fg, 1] = 0.0
    bg_pts[kink[~is_fg], 0] = means[~is_fg][kink[~is_fg], 0]
    prev_col[kink, 2] = col[kink, 2]
    variables = {"init_bg_pts": bg_pts.contiguous(), "init_bg_rot": bg_rot.contiguous(), "prev_col": prev_col}
    return means, raw, col, is_fg, variables


def _tables(P, frac, raw_rotations):
    means, raw, col, is_fg, variables = _case(P, frac)
    return means, raw if raw_rotations else torch.nn.functional.normalize(raw), col, is_fg, variables


def _total(losses, dtype, device):
    up = torch.tensor(UP, dtype=dtype, device=device)
    return sum(l * u for l, u in zip(losses, up))  # a NaN loss leaves the other terms' gradients alone


@functools.lru_cache(maxsize=None)
def _reference(P, frac, raw_rotations):
    """regularizer_losses_torch in fp64 on the CPU: (losses, gradients of sum_k UP[k] * loss[k])."""
    means, rot, col, is_fg, variables = _tables(P, frac, raw_rotations)
    t = [x.double().requires_grad_(True) for x in (means, rot, col)]
    losses = regularizer_losses_torch(*t, {k: v.double() for k, v in variables.items()}, is_fg,
                                      raw_rotations=raw_rotations)
    grads = torch.autograd.grad(_total(losses, torch.float64, "cpu"), t)
    return [l.detach() for l in losses], grads


def _run_hip(tables, variables, is_fg, raw_rotations, split=None):
    t = [x.to(DEV).requires_grad_(True) if not x.is_cuda else x for x in tables]
    v = {k: x.to(DEV) for k, x in variables.items()}
    split = split or foreground_split(is_fg.to(DEV))
    losses = regularizer_losses(*t, v, split, raw_rotations=raw_rotations)
    grads = torch.autograd.grad(_total(losses, torch.float32, DEV), t)
    return [l.detach() for l in losses], grads


def _check_losses(got, want, tag):
    for name, g, w in zip(("floor", "bg", "soft_col_cons"), got, want):
        g, w = float(g), float(w)
        if np.isnan(w):
            assert np.isnan(g), (tag, name, g)
            continue
        err = abs(g - w) / max(abs(w), 1e-300)
        print(f"{tag}: {name} {g:.8f} (fp64 {w:.8f}) rel {err:.2e} of {LOSS_TOL:.0e}")
        assert err <= LOSS_TOL, (tag, name, g, w)


@pytest.mark.parametrize("raw_rotations", [False, True])
@pytest.mark.parametrize("frac", FRACTIONS)
@pytest.mark.parametrize("P", SIZES)
def test_losses_and_gradients_against_fp64(P, frac, raw_rotations):
    means, rot, col, is_fg, variables = _tables(P, frac, raw_rotations)
    want_l, want_g = _reference(P, frac, raw_rotations)
    got_l, got_g = _run_hip((means, rot, col), variables, is_fg, raw_rotations)
    tag = f"P={P} fg={int(is_fg.sum())} raw={raw_rotations}"
    _check_losses(got_l, want_l, tag)
    for name, g, w in zip(TABLES, got_g, want_g):
        assert g.shape == w.shape and g.dtype == torch.float32 and torch.isfinite(g).all()
        tol = RAW_GRAD_TOL if (raw_rotations and name == "rotations") else GRAD_TOL
        if not w.any():
            assert not g.any(), (tag, name)  # e.g. the rotations with no background
            continue
        err = _rel(g, w)
        print(f"{tag}: d{name} rel L2 {err:.2e} of {tol:.1e}")
        assert err <= tol, (tag, name)
        if tol == GRAD_TOL:  # +-g/N or 0, element for element
            assert torch.equal(torch.sign(g).cpu(), torch.sign(w).float()), (tag, name)


@pytest.mark.parametrize("raw_rotations", [False, True])
def test_views_four_bytes_past_a_16_byte_boundary_take_the_scalar_path(raw_rotations):
    """A parameter that is a view into a flat buffer is only 4-byte aligned: same bits as the
    aligned call."""
    P = 257
    means, rot, col, is_fg, variables = _tables(P, 0.4, raw_rotations)

    def shifted(x):
        flat = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)
        view = flat[1:].view(x.shape)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view.detach().requires_grad_(True)

    base_l, base_g = _run_hip((means, rot, col), variables, is_fg, raw_rotations)
    v_shift = {k: shifted(x).detach() for k, x in variables.items()}
    got_l, got_g = _run_hip((shifted(means), shifted(rot), shifted(col)), v_shift, is_fg, raw_rotations)
    for a, b in zip(got_l + list(got_g), base_l + list(base_g)):
        assert torch.equal(a, b)
    _check_losses(got_l, _reference(P, 0.4, raw_rotations)[0], f"shifted raw={raw_rotations}")
    # the gather reads the same views
    split = foreground_split(is_fg.to(DEV))
    m, q = shifted(means), shifted(rot)
    fg_pts, fg_rot = gather_foreground(m, q, split)
    assert torch.equal(fg_pts, m.detach()[split.is_fg]) and torch.equal(fg_rot, q.detach()[split.is_fg])


def test_kink_rows_of_the_fixture_match_in_sign_and_zero():
    gold = np.load(GOLD)
    t = lambda k: torch.from_numpy(gold[f"tiny.{k}"])  # noqa: E731
    variables = {k: t(k) for k in ("init_bg_pts", "init_bg_rot", "prev_col")}
    tables = [t(k).to(DEV).requires_grad_(True) for k in TABLES]
    split = foreground_split(t("is_fg").to(DEV))
    losses = regularizer_losses(*tables, {k: v.to(DEV) for k, v in variables.items()}, split)
    up = torch.tensor(gold["tiny.up"], dtype=torch.float32, device=DEV)
    grads = torch.autograd.grad(sum(l * u for l, u in zip(losses, up)), tables)
    _check_losses([l.detach() for l in losses], gold["tiny.losses"], "tiny")
    for k, g in zip(TABLES, grads):
        ref = gold[f"tiny.grad_{k}"]
        assert np.array_equal(np.sign(g.cpu().numpy()), np.sign(ref)), k
        assert _rel(g, torch.from_numpy(ref)) <= GRAD_TOL, k
    g = grads[0].cpu()
    assert g[0, 1] > 0 and g[2, 1] == 0 and g[3, 2] == 0 and grads[2][4, 0] == 0  # y == 0 passes; |0| gives 0


@pytest.mark.parametrize("P,frac", [(257, 0.4), (1000, 0.4), (P_LOOPED, 0.4), (65, 1.0)])
def test_means_and_colour_gradients_equal_torch_fp32_autograd_on_the_device(P, frac):
    """The share of a row in a mean's gradient is g * (1 / N) with the reciprocal rounded to fp32
    first: what torch's device kernel computes for a division by a host scalar.  Bit for bit."""
    means, rot, col, is_fg, variables = _tables(P, frac, False)
    t = [x.to(DEV).requires_grad_(True) for x in (means, rot, col)]
    v = {k: x.to(DEV) for k, x in variables.items()}
    ref_l = regularizer_losses_torch(*t, v, is_fg.to(DEV))
    ref_g = torch.autograd.grad(_total(ref_l, torch.float32, DEV), t)
    _, got_g = _run_hip(t, variables, is_fg, False)
    assert torch.equal(got_g[0], ref_g[0]), "means3D"
    assert torch.equal(got_g[2], ref_g[2]), "rgb_colors"
    print(f"P={P}: rotations gradient equal to torch's: {torch.equal(got_g[1], ref_g[1])}")


@pytest.mark.parametrize("P,frac", [(1, 1.0), (1, 0.0), (65, 0.4), (257, 0.0), (257, 1.0), (5000, 0.4)])
def test_gather_foreground_is_boolean_indexing_bit_for_bit(P, frac):
    gen = torch.Generator().manual_seed(P)
    means, rot = torch.randn(P, 3, generator=gen), torch.randn(P, 4, generator=gen)
    is_fg = (torch.rand(P, generator=gen) < frac if 0.0 < frac < 1.0 else torch.full((P,), frac == 1.0)).to(DEV)
    split = foreground_split(is_fg)
    a = [x.to(DEV).requires_grad_(True) for x in (means, rot)]
    b = [x.to(DEV).requires_grad_(True) for x in (means, rot)]
    fg_pts, fg_rot = gather_foreground(*a, split)
    want_pts, want_rot = b[0][is_fg], b[1][is_fg]
    assert fg_pts.shape == (split.n_fg, 3) and fg_rot.shape == (split.n_fg, 4)
    assert torch.equal(fg_pts, want_pts) and torch.equal(fg_rot, want_rot)
    gen = torch.Generator(device=DEV).manual_seed(3)
    up_p = torch.randn(split.n_fg, 3, device=DEV, generator=gen)
    up_r = torch.randn(split.n_fg, 4, device=DEV, generator=gen)
    got = torch.autograd.grad([fg_pts, fg_rot], a, [up_p, up_r])
    want = torch.autograd.grad([want_pts, want_rot], b, [up_p, up_r])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].shape == (P, 3) and not got[0][~is_fg].any() and not got[1][~is_fg].any()
    # one output used: the other table's gradient is all zeros, written, not left over
    fg_pts, _ = gather_foreground(*a, split)
    only = torch.autograd.grad(fg_pts.sum(), a, allow_unused=True)
    assert torch.equal(only[0], is_fg[:, None].float().expand(P, 3)) and (only[1] is None or not only[1].any())


def test_two_runs_are_bit_identical():
    means, rot, col, is_fg, variables = _tables(P_LOOPED, 0.4, True)
    runs = [_run_hip((means, rot, col), variables, is_fg, True) for _ in range(2)]
    for a, b in zip(runs[0][0] + list(runs[0][1]), runs[1][0] + list(runs[1][1])):
        assert torch.equal(a, b)


def test_cpu_tensors_raise():
    means, rot, col, is_fg, variables = _tables(65, 0.4, False)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        regularizer_losses(means, rot, col, variables, foreground_split(is_fg))
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        gather_foreground(means.to(DEV), rot, foreground_split(is_fg.to(DEV)))


# ------------------------------------------------------------ the reference's block, end to end

N_FG, P_SCENE, K = 2000, 5000, 20


@functools.lru_cache(maxsize=None)
def _scene():
    """P = 5000 rows, 2000 of them foreground with the neighbour state of tests/test_neighbor.py
    (k = 20 graph, previous-timestep offsets and rotations, the current state moved a little)."""
    gen = torch.Generator().manual_seed(77)
    fg_pts, fg_rot, graph = make_state(N=N_FG, K=K, seed=7)
    is_fg = torch.zeros(P_SCENE, dtype=torch.bool)
    is_fg[torch.randperm(P_SCENE, generator=gen)[:N_FG]] = True
    means = 0.3 * torch.randn(P_SCENE, 3, generator=gen)
    means[is_fg] = fg_pts
    unnorm = torch.nn.functional.normalize(torch.randn(P_SCENE, 4, generator=gen))
    unnorm[is_fg] = fg_rot
    unnorm = unnorm * (0.5 + torch.rand(P_SCENE, 1, generator=gen))
    col = torch.rand(P_SCENE, 3, generator=gen)
    seg = torch.zeros(P_SCENE, 3)
    seg[:, 0] = is_fg.float()
    n_bg = P_SCENE - N_FG
    variables = dict(graph)
    variables["init_bg_pts"] = means[~is_fg] + 0.02 * torch.randn(n_bg, 3, generator=gen)
    variables["init_bg_rot"] = torch.nn.functional.normalize(
        torch.nn.functional.normalize(unnorm[~is_fg]) + 0.02 * torch.randn(n_bg, 4, generator=gen))
    variables["prev_col"] = col + 0.02 * torch.randn(P_SCENE, 3, generator=gen)
    return {"means3D": means, "unnorm_rotations": unnorm, "rgb_colors": col, "seg_colors": seg}, variables


def _device_scene():
    base, variables = _scene()
    params = {k: v.to(DEV).requires_grad_(k != "seg_colors") for k, v in base.items()}
    return params, {k: v.to(DEV).contiguous() for k, v in variables.items()}


def _rendervar(params):
    return {"means3D": params["means3D"], "rotations": torch.nn.functional.normalize(params["unnorm_rotations"])}


def _boolean_block(params, variables, rv, t, w):
    """The block as a caller must write it without scene_loss: boolean indexing, neighbor_losses,
    the torch terms."""
    is_fg = (params["seg_colors"][:, 0] > 0.5).detach()
    rigid, rot, iso = neighbor_losses(rv["means3D"][is_fg], rv["rotations"][is_fg], variables)
    floor, bg, col = regularizer_losses_torch(rv["means3D"], rv["rotations"], params["rgb_colors"], variables, is_fg)
    return (w["rigid"] * rigid + w["rot"] * rot + w["iso"] * iso + w["floor"] * floor + w["bg"] * bg
            + w["soft_col_cons"] * col)


LEAVES = ("means3D", "unnorm_rotations", "rgb_colors")
WEIGHTS = {"rigid": 0.4, "rot": 0.4, "iso": 0.2, "floor": 0.2, "bg": 2.0, "soft_col_cons": 0.01}


def test_reference_extra_loss_end_to_end():
    fn = reference_extra_loss()
    params, variables = _device_scene()
    assert fn(params, variables, _rendervar(params), 0) is None
    assert fn(params, {k: v for k, v in variables.items() if k != "neighbor_indices"}, _rendervar(params), 1) is None
    got = fn(params, variables, _rendervar(params), 1)
    got_g = torch.autograd.grad(got, [params[k] for k in LEAVES])
    ref_p, ref_v = _device_scene()
    want = _boolean_block(ref_p, ref_v, _rendervar(ref_p), 1, WEIGHTS)
    want_g = torch.autograd.grad(want, [ref_p[k] for k in LEAVES])
    err = abs(got.item() - want.item()) / abs(want.item())
    print(f"extra loss {got.item():.8f} (boolean indexing {want.item():.8f}) rel {err:.2e} of {LOSS_TOL:.0e}")
    assert want.item() > 0 and err <= LOSS_TOL
    for k, g, w in zip(LEAVES, got_g, want_g):
        e = _rel(g, w)
        print(f"d{k}: rel L2 {e:.2e} of 1e-4")
        assert w.abs().sum() > 0 and e <= 1e-4, k
    # twice: the same bits
    again = torch.autograd.grad(fn(params, variables, _rendervar(params), 1), [params[k] for k in LEAVES])
    for a, b in zip(again, got_g):
        assert torch.equal(a, b)


def test_reference_extra_loss_makes_no_host_sync():
    """torch.cuda.set_sync_debug_mode("error") raises at every call that makes the host wait for
    the device.  Armed on the boolean-indexing formulation first, which must raise."""
    fn = reference_extra_loss()
    params, variables = _device_scene()
    ref_p, ref_v = _device_scene()
    leaves = [params[k] for k in LEAVES]
    # warm-ups outside the mode: the split, the mask and the reverse CSR are built and cached
    torch.autograd.grad(fn(params, variables, _rendervar(params), 1), leaves)
    torch.autograd.grad(_boolean_block(ref_p, ref_v, _rendervar(ref_p), 1, WEIGHTS), [ref_p[k] for k in LEAVES])
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            _boolean_block(ref_p, ref_v, _rendervar(ref_p), 1, WEIGHTS)
            armed = False
        except RuntimeError as e:
            armed = "synchroniz" in str(e)
        if armed:
            loss = fn(params, variables, _rendervar(params), 1)
            grads = torch.autograd.grad(loss, leaves)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not armed:
        pytest.skip("this torch build's sync debug mode does not see boolean indexing: nothing to check against")
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads)
