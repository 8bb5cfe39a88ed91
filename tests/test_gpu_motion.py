"""The motion-basis warp (csrc/gs_motion.hip) on the GPU against
motion_positions_torch in fp64 on the CPU -- never the code under test.

Bounds (the project's convention, tests/test_gpu_image_loss.py): outputs within
1e-5 * max(1, |ref|) per element, every gradient within 1e-4 relative L2, and
d_rots, d_transls, d_coefs within 10x the error of the reference formulation
itself in fp32 (motion_positions_torch in fp32 on the CPU against fp64,
computed here).  Every case is built by the fixture's recipe and keeps its
conditioning margin (tests/_motion_cases.py), asserted here.

Shapes: one thread per Gaussian in workgroups of 256 (128 at K = 64, B = 32,
where 256 columns would not fit the LDS); the backward sums 16 interleaved
segments of per-workgroup slabs.  So: G = 1; G = 257 (two workgroups, one
Gaussian in the second) with K = 1, B = 1; G = 1000 with unsorted ts and a
repeated frame; K = 64, B = 32 (the LDS envelope, 128-thread workgroups, a
ragged third one); G = 20003 at K = 20, B = 6 (79 slabs: every segment loops,
ragged tail); and the two fixture cases.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (MotionBases, _lib, motion_positions, motion_positions_torch,
                                    motion_transforms)
from tests import _harness as H
from tests import _motion_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUT_TOL, GRAD_TOL, ENVELOPE = 1e-5, 1e-4, 10.0

# name: (G, K, T, ts, first seed)
SEEDED = {
    "one": (1, 5, 10, (4, 0, 9, 2), 11),
    "k1b1": (257, 1, 3, (1,), 13),
    "unsorted": (1000, 7, 12, (7, 2, 11, 2, 0, 9, 5, 3, 10), 11),  # frame 2 twice
    "envelope": (300, 64, 40, tuple((7 * i + 3) % 40 for i in range(32)), 12),
    "slabs": (20003, 20, 8, (5, 1, 7, 0, 3, 6), 11),
    "chunks": (300, 3, 50, tuple((11 * i + 5) % 50 for i in range(38)) + (5, 16), 28),  # 40 frames, two repeated
}
PARITY = ("c200", "c64", "one", "k1b1", "unsorted", "envelope", "slabs")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, ts): fp64 CPU tensors of fp32-representable values."""
    if name in mc.FIXTURE_CASES:
        gold = np.load(mc.GOLD)
        case = {k: torch.from_numpy(gold[f"{name}.{k}"]) for k in ("means", "logits", "coefs", "rots", "transls")}
        ts = tuple(gold[f"{name}.ts"].tolist())
    else:
        G, K, T, ts, seed = SEEDED[name]
        case, _ = mc.conditioned_case(G, K, T, ts, seed)
    for softmax in (False, True):
        assert mc.margins_ok(case, ts, softmax), (name, mc.margins(case, ts, softmax))
    return case, ts


def _run(impl, name, softmax, entry, dtype, dev):
    """(output, [d_means,] d_coefs, d_rots, d_transls) of sum(w * output)."""
    case, ts = _case(name)
    mv = lambda k: case[k].to(device=dev, dtype=dtype).requires_grad_(True)  # noqa: E731
    means, coefs, rots, transls = mv("means"), mv("logits" if softmax else "coefs"), mv("rots"), mv("transls")
    if impl == "torch":
        pos, tf = motion_positions_torch(means, coefs, rots, transls, ts, softmax=softmax, return_transforms=True)
        out = pos if entry == "positions" else tf
    elif entry == "positions":
        out = motion_positions(means, coefs, rots, transls, ts, softmax=softmax)
    else:
        out = motion_transforms(coefs, rots, transls, ts, softmax=softmax)
    w = mc.weights(means.shape[0], len(ts), 5, transforms=entry == "transforms").to(device=dev, dtype=dtype)
    wrt = ([means] if entry == "positions" else []) + [coefs, rots, transls]
    grads = torch.autograd.grad((w * out).sum(), wrt)
    return [out.detach()] + list(grads)


@functools.lru_cache(maxsize=None)
def _oracle(name, softmax, entry):
    """The fp64 CPU oracle and the fp32 CPU formulation's own relative L2 errors against it."""
    ref = _run("torch", name, softmax, entry, torch.float64, "cpu")
    f32 = _run("torch", name, softmax, entry, torch.float32, "cpu")
    return ref, [mc.rel_l2(a, b) if bool(b.any()) else float(a.abs().max()) for a, b in zip(f32, ref)]


def _check(name, softmax, entry):
    ref, ref32 = _oracle(name, softmax, entry)
    got = _run("hip", name, softmax, entry, torch.float32, DEV)
    torch.cuda.synchronize()
    got = [g.double().cpu() for g in got]
    names = ["out"] + (["d_means"] if entry == "positions" else []) + ["d_coefs", "d_rots", "d_transls"]
    assert got[0].shape == ref[0].shape
    out_err = ((got[0] - ref[0]).abs() / ref[0].abs().clamp_min(1.0)).max().item() if ref[0].numel() else 0.0
    line = [f"{name} softmax={softmax} {entry}: out err {out_err:.2e}"]
    assert out_err <= OUT_TOL
    for n, g, r, e32 in list(zip(names, got, ref, ref32))[1:]:
        assert g.shape == r.shape and torch.isfinite(g).all(), n
        if not bool(r.any()):  # one basis under softmax: the logit's gradient is exactly zero
            assert n == "d_coefs" and softmax and r.shape[1] == 1
            assert not bool(g.any()), "d_logits of a single basis must be exactly 0"
            line.append(f"{n} exactly 0")
            continue
        err = mc.rel_l2(g, r)
        line.append(f"{n} {err:.2e} (fp32 formulation {e32:.2e}, ratio {err / e32:.2f})")
        assert err <= GRAD_TOL, (n, err)
        if n != "d_means":
            assert err <= ENVELOPE * e32, (n, err, e32)
    print("; ".join(line))
    return got, ref


@pytest.mark.parametrize("entry", ("positions", "transforms"))
@pytest.mark.parametrize("softmax", (False, True), ids=("given", "softmax"))
@pytest.mark.parametrize("name", PARITY)
def test_value_and_gradient_parity(name, softmax, entry):
    got, ref = _check(name, softmax, entry)
    case, ts = _case(name)
    T = case["rots"].shape[1]
    rest = [t for t in range(T) if t not in ts]
    d_rots, d_transls = got[-2], got[-1]
    # rows of frames outside ts are exactly zero, not merely small
    assert not bool(d_rots[:, rest].any()) and not bool(d_transls[:, rest].any())
    if name in mc.FIXTURE_CASES and entry == "positions":  # the same oracle as the committed reference outputs
        gold = np.load(mc.GOLD)
        mode = "softmax" if softmax else "given"
        assert np.abs(got[0].numpy() - gold[f"{name}.{mode}.positions"]).max() <= OUT_TOL * \
            max(1.0, np.abs(gold[f"{name}.{mode}.positions"]).max())


def test_a_repeated_frame_receives_the_sum_of_its_occurrences():
    got, ref = _check("unsorted", True, "positions")
    d_rots = got[-2]
    # frame 2 is ts[1] and ts[3]: the oracle's row is the sum of both; it differs from either alone
    case, ts = _case("unsorted")
    assert ts.count(2) == 2
    assert mc.rel_l2(d_rots[:, 2], ref[-2][:, 2]) <= GRAD_TOL
    assert mc.rel_l2(got[-1][:, 2], ref[-1][:, 2]) <= GRAD_TOL


def test_forty_frames_run_as_two_chunks():
    """ts of 40 frames (more than one call takes), two of them repeated across the chunk boundary."""
    case, ts = _case("chunks")
    assert len(ts) == 40 and ts.count(5) == 2 and ts.index(5) < 32 <= 38 + ts[38:].index(5)
    for entry in ("positions", "transforms"):
        got, ref = _check("chunks", True, entry)
        assert got[0].shape[1] == 40


def _raw(name, softmax, fill, shift=0, bwd=True):
    """The C ABI called directly on buffers prefilled with `fill`: (positions, transforms, d_means,
    d_coefs, d_rots, d_transls).  `shift` floats of offset put the transforms and their gradient
    off 16-byte alignment (the scalar paths)."""
    L = _lib.load()
    case, ts = _case(name)
    f = lambda k: case[k].float().to(DEV).contiguous()  # noqa: E731
    means, coefs, rots, transls = f("means"), f("logits" if softmax else "coefs"), f("rots"), f("transls")
    G, K = coefs.shape
    B = len(ts)
    d = _lib.GsMotionDesc(G=G, K=K, T=rots.shape[1], B=B, coef_mode=int(softmax), rots=rots.data_ptr(),
                          transls=transls.data_ptr(), coefs=coefs.data_ptr(), means=means.data_ptr())
    for b, t in enumerate(ts):
        d.ts[b] = t
    full = lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV)  # noqa: E731
    pos = full(G, B, 3)
    tf_buf = full(G * B * 12 + 4)
    tf = tf_buf[shift:shift + G * B * 12]
    assert tf.data_ptr() % 16 == (4 * shift) % 16
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(L.gs_motion_forward(d, pos.data_ptr(), tf.data_ptr(), None, stream), "forward")
    outs = [pos, tf.view(G, B, 3, 4).clone()]
    if bwd:
        w_pos = mc.weights(G, B, 5).float().to(DEV)
        w_buf = full(G * B * 12 + 4)
        w_tf = w_buf[shift:shift + G * B * 12]
        w_tf.copy_(mc.weights(G, B, 6, transforms=True).float().reshape(-1))
        d_means, d_coefs, d_rots, d_transls = full(G, 3), full(G, K), full(*rots.shape), full(*transls.shape)
        ws = torch.full((L.gs_motion_workspace_bytes(G, K, B, 1) // 4,), fill, dtype=torch.float32, device=DEV)
        _lib.check(L.gs_motion_backward(d, w_pos.data_ptr(), w_tf.data_ptr(), d_means.data_ptr(), d_coefs.data_ptr(),
                                        d_rots.data_ptr(), d_transls.data_ptr(), ws.data_ptr(), stream), "backward")
        outs += [d_means, d_coefs, d_rots, d_transls]
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("name", ("unsorted", "slabs"))
def test_outputs_are_written_not_accumulated_and_runs_are_bit_identical(name):
    """Every output and the workspace start as NaN, then as 1e30: a buffer that was added to, or a
    workspace word read before it was written, shows; and the two runs agree bit for bit (fixed
    summation order, no atomics).  Both upstream gradients at once: dR and dt take both terms."""
    a = _raw(name, True, float("nan"))
    b = _raw(name, True, 1e30)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
    # both upstream gradients together equal the sum of the two entry points' oracles
    case, ts = _case(name)
    lv = lambda k: case[k].clone().requires_grad_(True)  # noqa: E731
    means, logits, rots, transls = lv("means"), lv("logits"), lv("rots"), lv("transls")
    pos, tf = motion_positions_torch(means, logits, rots, transls, ts, softmax=True, return_transforms=True)
    G, B = pos.shape[:2]
    loss = (mc.weights(G, B, 5) * pos).sum() + (mc.weights(G, B, 6, transforms=True) * tf).sum()
    ref = torch.autograd.grad(loss, (means, logits, rots, transls))
    for n, g, r in zip(("d_means", "d_coefs", "d_rots", "d_transls"), a[2:], ref):
        assert mc.rel_l2(g, r) <= GRAD_TOL, n


def test_unaligned_transforms_take_the_scalar_path_and_agree_bitwise():
    a = _raw("unsorted", False, float("nan"), shift=0)
    b = _raw("unsorted", False, float("nan"), shift=1)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_no_gaussians():
    case = mc.make_case(4, 3, 5, 3)
    f = lambda k, n: case[k][:n].float().to(DEV).requires_grad_(True)  # noqa: E731
    means, coefs = f("means", 0), f("logits", 0)
    rots, transls = f("rots", 3), f("transls", 3)
    pos = motion_positions(means, coefs, rots, transls, [4, 1], softmax=True)
    tf = motion_transforms(coefs, rots, transls, [4, 1], softmax=True)
    assert pos.shape == (0, 2, 3) and tf.shape == (0, 2, 3, 4)
    (pos.sum() + tf.sum()).backward()
    torch.cuda.synchronize()
    assert rots.grad.shape == (3, 5, 6) and not bool(rots.grad.any()) and not bool(transls.grad.any())
    assert means.grad.shape == (0, 3) and coefs.grad.shape == (0, 3)
    # the C ABI, on NaN-filled tables: zeroed, nothing else needed
    L = _lib.load()
    d_rots = torch.full((3, 5, 6), float("nan"), device=DEV)
    d_transls = torch.full((3, 5, 3), float("nan"), device=DEV)
    d = _lib.GsMotionDesc(G=0, K=3, T=5, B=2, coef_mode=1, rots=rots.data_ptr(), transls=transls.data_ptr())
    d.ts[0], d.ts[1] = 4, 1
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(L.gs_motion_forward(d, None, ctypes.c_void_p(16), None, stream), "empty forward")
    _lib.check(L.gs_motion_backward(d, None, None, None, None, d_rots.data_ptr(), d_transls.data_ptr(), None, stream),
               "empty backward")
    torch.cuda.synchronize()
    assert not bool(d_rots.any()) and not bool(d_transls.any())


def test_wrapper_accepts_device_ts_and_rejects_what_the_kernels_cannot_take():
    case, ts = _case("one")
    f = lambda k: case[k].float().to(DEV)  # noqa: E731
    means, coefs, rots, transls = f("means"), f("coefs"), f("rots"), f("transls")
    want = motion_positions(means, coefs, rots, transls, list(ts))
    for form in (torch.tensor(ts, device=DEV), torch.tensor(ts, dtype=torch.int32), [t - 10 for t in ts]):
        assert torch.equal(motion_positions(means, coefs, rots, transls, form), want)
    with pytest.raises(IndexError):
        motion_positions(means, coefs, rots, transls, [10])
    big = mc.make_case(3, 65, 2, 1)
    with pytest.raises(ValueError, match="at most 64"):
        motion_positions(*(big[k].float().to(DEV) for k in ("means", "coefs", "rots", "transls")), [0])
    # non-fp32 device inputs take the torch formulation
    out = motion_positions(means.double(), coefs.double(), rots.double(), transls.double(), list(ts))
    assert out.dtype == torch.float64 and mc.rel_l2(out, want) <= 1e-5


def test_motion_bases_feed_the_rasterizer_end_to_end():
    """MotionBases.compute_means -> means3D of one 64 x 64 camera -> GaussianRasterizer; the backward
    reaches the logits and both bases.  Against the same render fed by the torch formulation."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = H.scene(P=600, F=32, W=64, H=64)
    P, K, T = 600, 4, 3
    gen = torch.Generator().manual_seed(3)
    ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0])
    rots0 = (ident + 0.05 * torch.randn(K, T, 6, generator=gen)).to(DEV)
    transls0 = (0.05 * torch.randn(K, T, 3, generator=gen)).to(DEV)
    logits0 = (2.0 * torch.randn(P, K, generator=gen)).to(DEV)
    wc = torch.randn(3, 64, 64, generator=gen).to(DEV)
    wf = torch.randn(32, 64, 64, generator=gen).to(DEV)
    s = GaussianRasterizationSettings(
        image_height=64, image_width=64, tanfovx=inp["tan_fovx"], tanfovy=inp["tan_fovy"], c_x=inp["c_x"],
        c_y=inp["c_y"], bg=torch.zeros(3, device=DEV), scale_modifier=1.0, viewmatrix=inp["viewmatrix"].to(DEV),
        projmatrix=inp["projmatrix"].to(DEV), sh_degree=0, campos=inp["campos"].to(DEV), prefiltered=False,
        debug=False, confidence=None)

    def render(fused):
        bases = MotionBases(rots0, transls0)
        assert bases.params["rots"].is_cuda
        means = inp["means3D"].to(DEV).requires_grad_(True)
        logits = logits0.clone().requires_grad_(True)
        if fused:
            xyz = bases.compute_means([2, 1], means, logits, softmax=True)[:, 1].contiguous()
        else:
            xyz = motion_positions_torch(means, logits, bases.params["rots"], bases.params["transls"], [2, 1],
                                         softmax=True)[:, 1].contiguous()
        im, radii, feat, depth, alpha = GaussianRasterizer(s)(
            means3D=xyz, means2D=torch.zeros_like(xyz, requires_grad=True), opacities=inp["opacity"].to(DEV),
            colors_precomp=inp["colors"].to(DEV), scales=inp["scales"].to(DEV), rotations=inp["rotations"].to(DEV),
            semantic_feature=inp["semantic_feature"].to(DEV), label=torch.ones(P, device=DEV))
        ((im * wc).sum() + (feat * wf).mean()).backward()
        torch.cuda.synchronize()
        return im.detach().cpu(), [t.grad.detach().cpu() for t in (means, logits, bases.params["rots"],
                                                                  bases.params["transls"])]

    im_a, grads_a = render(True)
    im_b, grads_b = render(False)
    assert float(im_b.abs().max()) > 0.1 and ((im_a - im_b).abs() <= OUT_TOL * im_b.abs().clamp_min(1.0)).all()
    for n, a, b in zip(("means", "logits", "rots", "transls"), grads_a, grads_b):
        assert bool(b.any()), n
        err = mc.rel_l2(a, b)
        print(f"end to end d_{n}: {err:.2e}")
        assert err <= GRAD_TOL, (n, err)
    assert not bool(grads_a[2][:, 0].any())  # frame 0 was not asked for
