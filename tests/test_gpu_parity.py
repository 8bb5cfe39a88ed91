"""GPU parity: the HIP rasterizer (through the C ABI) against the CPU oracle.

Tolerances (DESIGN.md section 5 has the measured errors):
  * integer/index work (tile counts, sorted point lists, tile ranges, radii,
    the radix sort, the wave reduction on integer data): bit-exact;
  * preprocess floats (means2D, depths, conics, SH colours): bit-exact -- both
    sides are strict IEEE fp32 in the same operation order;
  * rendered images: PSNR(HIP vs oracle) >= 80 dB and >= 99.9 % of pixels
    within 1e-5 absolute on colour, feature (and alpha) channels, depth within
    1e-5 relative to the depth range; n_contrib identical for >= 99.9 % of
    pixels (the blend's exp is v_exp_f32, not libm expf, so an
    alpha-threshold decision may flip on a rare pixel).  Measured: colour
    <= 4.8e-7, features <= 2.9e-6 (3-piece bf16 split contractions);
  * gradients: relative L2 over all Gaussians <= 1e-4 per output tensor
    (measured <= 2.1e-5, typically ~1e-6), and -- test_gpu_envelope -- within
    10x the oracle's own fp32 summation-order spread in reference mode.

These aggregate bars hold on full-size scenes, where a decision may flip on a
rare pixel.  tests/test_gpu_elementwise.py adds the per-element guarantee on
decision-robust scenes (tests/_robust.py; margin factor 8): every pixel and
every Gaussian within 10 K u A of the fp64 replay of the blend, A its own
absolute sum.  K_oracle (the fp32 C oracle's own worst) / HIP worst measured:
colour 21 / 15.1, features 30 / 18.3, depth 18 / 17.5, alpha 3.4 / 3.3,
dmeans2D 6.2 / 24.6, dopacity 6.6 / 10.1, dcolors 27 / 58.8, dsemantic
51 / 79.4; behind preprocess_bwd K_down 154, HIP worst 435 (in units of
u |J| A); same last contributor at every pixel.
"""
import numpy as np
import pytest
import torch

from tests import _harness as H
from dynamic3dgaussians_amd import _C, _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _cmp_forward(inp, compat, F):
    g = H.gpu_forward(inp, compat)
    o = H.oracle_forward(inp, compat)
    Lg, cg, fg, dg, ag, rg = g[0], g[1].cpu().numpy(), g[2].cpu().numpy(), g[3].cpu().numpy(), \
        g[4].cpu().numpy(), g[5].cpu().numpy()
    Lo, co, fo, do, ao, ro, st = o
    assert Lg == Lo, "num_rendered differs"
    np.testing.assert_array_equal(rg, ro)
    assert H.psnr(cg, co) >= 80.0
    assert np.mean(np.abs(cg - co) <= 1e-5) >= 0.999
    assert np.mean(np.abs(dg - do) <= 1e-5 * max(1.0, np.abs(do).max())) >= 0.999
    if F:
        assert fg.shape == fo.shape
        assert np.mean(np.abs(fg - fo) <= 1e-5) >= 0.999
    assert np.mean(np.abs(ag - ao) <= 1e-5) >= 0.999
    return g, o


# ---------------------------------------------------------------- primitives

@pytest.mark.parametrize("n", [1, 2, 3, 10, 13, 18, 26, 42, 64])
def test_wave_transposed_reduce(n):
    L = _lib.load()
    rng = np.random.default_rng(n)
    x = rng.integers(-1000, 1000, size=(n, 64)).astype(np.float32)  # exact sums
    xin = torch.from_numpy(x).cuda()
    out = torch.full((n,), np.nan, device="cuda")
    _lib.check(L.gs_test_wave_reduce(n, xin.data_ptr(), out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "wave reduce")
    np.testing.assert_array_equal(out.cpu().numpy(), x.sum(1))


@pytest.mark.parametrize("n,end_bit", [(0, 40), (1, 40), (777, 40), (4096, 44), (100_000, 44),
                                       (1_000_003, 45), (50_000, 13)])
def test_radix_sort_stable(n, end_bit):
    """Bit-exact against numpy's stable argsort on the sorted bit range,
    with heavy key duplication (stability matters)."""
    L = _lib.load()
    rng = np.random.default_rng(n + end_bit)
    tiles = rng.integers(0, 1 << max(end_bit - 32, 1), size=n, dtype=np.uint64)
    depth = rng.integers(0x3f800000, 0x3f800000 + 5000, size=n, dtype=np.uint64)
    keys = (tiles << np.uint64(32)) | depth if end_bit > 32 else depth & np.uint64((1 << end_bit) - 1)
    vals = np.arange(n, dtype=np.uint32)
    kd = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    vd = torch.from_numpy(vals.view(np.int32).copy()).cuda()
    scratch = torch.empty(max(L.gs_sort_scratch_bytes(n), 1), dtype=torch.uint8, device="cuda")
    _lib.check(L.gs_sort_pairs(n, kd.data_ptr(), vd.data_ptr(), end_bit, scratch.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "sort")
    torch.cuda.synchronize()
    masked = keys & np.uint64((1 << end_bit) - 1) if end_bit < 64 else keys
    order = np.argsort(masked, kind="stable")
    np.testing.assert_array_equal(vd.cpu().numpy().view(np.uint32), vals[order])
    np.testing.assert_array_equal(kd.cpu().numpy().view(np.uint64), keys[order])


# ---------------------------------------------------------------- stages

@pytest.mark.parametrize("kw", [
    dict(), dict(use_sh=True, sh_degree=1), dict(use_sh=True, sh_degree=2),
    dict(use_sh=True, sh_degree=3), dict(use_cov=True), dict(W=100, H=75, cam_index=5),
    dict(cx=40.0, cy=70.0, W=128, H=96),
    # tiles longer than the LDS sort (> 8192 instances): the global-memory path
    dict(P=20000, W=48, H=32), dict(P=30000, W=48, H=32), dict(P=60000, W=80, H=48),
    # more tiles than one binning pass holds (TB_BINS = 16384): the count and
    # bucket passes run per tile range; workgroups above and below the staged
    # bucket's LDS capacity (direct and staged stores)
    dict(P=20000, W=2112, H=2080)])
def test_preprocess_and_binning_bitexact(kw):
    inp = H.scene(**{"P": 3000, **kw})
    g = H.gpu_forward(inp)
    o = H.oracle_forward(inp)
    st_o = o[6]
    P, W, Hh = inp["means3D"].shape[0], inp["image_width"], inp["image_height"]
    st_g = H.export_state(P, W, Hh, g)
    vis = st_o.radii > 0
    np.testing.assert_array_equal(g[5].cpu().numpy(), st_o.radii)
    np.testing.assert_array_equal(st_g["tiles"], st_o.tiles_touched)
    np.testing.assert_array_equal(st_g["means2D"][vis], st_o.means2D[vis])
    np.testing.assert_array_equal(st_g["depths"][vis], st_o.depths[vis])
    np.testing.assert_array_equal(st_g["conic_opacity"][vis], st_o.conic_opacity[vis])
    if kw.get("use_sh"):
        np.testing.assert_array_equal(st_g["rgb"][vis], st_o.rgb[vis])
    # binning: num_rendered is the reference's count, bit-exact; the tile
    # lists are the reference's lists (bit-exact order) minus the instances
    # that blend at no pixel of their tile
    assert g[0] == o[0]
    assert st_g["num_instances"] <= g[0]
    frac = H.check_tile_lists(st_g, st_o, W, Hh)
    assert 0.0 <= frac < 1.0


@pytest.mark.parametrize("mode", ["ties", "crowded", "ties_crowded", "groups"])
def test_binning_depth_ties_and_crowded_depths(mode):
    """The per-tile sort's two paths (gs_tiles.hip): the MSD bucket sort
    (each key placed by counting its bucket's smaller keys), and the radix
    sort it falls back to when a bucket holds more than 48 keys.  'ties':
    groups of Gaussians share a mean (bit-identical depths, so the list order
    inside a group is the Gaussian index, as the reference's stable sort
    leaves it); 'crowded': most means on a thin shell at one distance from
    the camera, a few elsewhere (most of a tile's keys in a few buckets of
    its span -- the radix path when the limit was a thread's run of buckets,
    the bucket sort since it is one bucket's keys); 'groups': disjoint
    groups of 2 .. 64 Gaussians on one mean each, around the 48-key bucket
    limit (47, 48, 49: one bucket of that many keys where only the group
    reaches), so both sides of the fallback boundary run (stats build:
    3 radix fallbacks among its tiles, none in the other modes)."""
    inp = H.scene(P=4000, W=96, H=64)
    m = inp["means3D"].clone()
    g = torch.Generator().manual_seed(3)
    if mode == "groups":
        perm = torch.randperm(m.shape[0], generator=g)
        o = 0
        for k in (2, 3, 8, 16, 47, 48, 49, 64):
            idx = perm[o:o + k]
            m[idx] = m[idx[0]].clone()
            o += k
    if "ties" in mode:
        src = torch.randint(0, m.shape[0], (m.shape[0] // 2,), generator=g)
        dst = torch.randperm(m.shape[0], generator=g)[: m.shape[0] // 2]
        m[dst] = m[src]
    if "crowded" in mode:
        # 90 % of the means on a thin shell around the camera, the rest where
        # they were: each tile's depth span is set by the few outliers while
        # most of its keys share one or two buckets
        c = inp["campos"].float()
        d = m - c
        r = d.norm(dim=1, keepdim=True)
        shell = c + d / r * r.median() * (1 + 1e-4 * torch.rand(m.shape[0], 1, generator=g))
        pick = torch.rand(m.shape[0], generator=g) < 0.9
        m = torch.where(pick[:, None], shell, m)
    inp["means3D"] = m.contiguous()
    gg = H.gpu_forward(inp)
    o = H.oracle_forward(inp)
    P, W, Hh = m.shape[0], inp["image_width"], inp["image_height"]
    st_g = H.export_state(P, W, Hh, gg)
    assert gg[0] == o[0]
    H.check_tile_lists(st_g, o[6], W, Hh)
    L = _lib.load(auto_build=False)
    if hasattr(L, "gs_sort_stats_read"):  # stats build: which sort path ran
        import ctypes
        buf = (ctypes.c_ulonglong * 2)()
        L.gs_sort_stats_read(buf)
        print(f"{mode}: tiles sorted in LDS {buf[0]}, radix fallbacks {buf[1]}")


# ---------------------------------------------------------------- forward

@pytest.mark.parametrize("compat", ["reference", "fixed"])
@pytest.mark.parametrize("kw", [
    dict(), dict(F=32), dict(F=8, use_sh=True, sh_degree=3), dict(F=16, use_cov=True),
    dict(F=64, W=80, H=48), dict(F=32, bg=(0.2, 0.5, 0.9)), dict(W=100, H=75, P=4000),
    dict(F=32, cx=30.0, cy=60.0), dict(F=3, bg=(0.2, 0.5, 0.9))])
def test_forward_parity(compat, kw):
    _cmp_forward(H.scene(**kw), compat, kw.get("F", 0))


def test_forward_padded_feature_width():
    """F = 5 is zero-padded to the 8-wide kernel; outputs keep 5 channels."""
    inp = H.scene(P=1500, F=5)
    g = H.gpu_forward(inp)
    o = H.oracle_forward(inp)
    assert g[2].shape == (5, 96, 128)
    np.testing.assert_allclose(g[2].cpu().numpy(), o[2], atol=1e-5, rtol=0)


# ---------------------------------------------------------------- backward

GRAD_NAMES = ["dmeans2D", "dcolors", "dsemantic", "dopacity", "dmeans3D", "dcov3D", "dsh",
              "dscales", "drotations"]


@pytest.mark.parametrize("compat", ["reference", "fixed"])
@pytest.mark.parametrize("kw", [
    dict(), dict(F=32), dict(F=8, use_sh=True, sh_degree=3), dict(F=16, use_cov=True),
    dict(F=32, bg=(0.3, 0.1, 0.7)), dict(W=100, H=75, P=4000, use_sh=True, sh_degree=1),
    dict(F=32, cx=30.0, cy=60.0), dict(F=3, bg=(0.3, 0.1, 0.7))])
def test_backward_parity(compat, kw):
    inp = H.scene(**kw)
    F = kw.get("F", 0)
    g = H.gpu_forward(inp, compat)
    o = H.oracle_forward(inp, compat)
    grads = H.upstream_grads(inp["image_height"], inp["image_width"], F)
    gb = H.gpu_backward(inp, g, grads, compat)
    ob = H.oracle_backward(inp, o, grads, compat)
    for name, a, b in zip(GRAD_NAMES, gb, ob):
        assert a.shape == b.shape, name
        if b.size == 0 or not np.any(b):
            assert not np.any(a) or np.abs(a).max() < 1e-6, name
            continue
        assert H.rel_l2(a, b) <= 1e-4, (name, H.rel_l2(a, b))


def test_backward_reference_swap_matters():
    """Q2: the reference's swapped camera arguments change dL/dscale a lot;
    the HIP path follows whichever order it is given, like the oracle."""
    inp = H.scene(F=0)
    g = H.gpu_forward(inp)
    o = H.oracle_forward(inp)
    grads = H.upstream_grads(96, 128, 0)
    a = H.gpu_backward(inp, g, grads, "reference", swap=True)
    b = H.oracle_backward(inp, o, grads, "reference", swap=True)
    c = H.gpu_backward(inp, g, grads, "reference", swap=False)
    assert H.rel_l2(a[7], b[7]) <= 1e-4
    assert H.rel_l2(a[7], c[7]) > 0.1


# ---------------------------------------------------------------- edge cases

def test_empty_and_culled():
    inp = H.scene(P=0)
    g = H.gpu_forward(inp)
    assert g[0] == 0 and g[1].abs().sum().item() == 0  # P == 0: no background either
    inp = H.scene(P=500, bg=(0.25, 0.5, 0.75))
    fwd = inp["viewmatrix"][:3, 2]  # camera forward axis (row 2 of w2c)
    inp["means3D"] = (inp["campos"] - 2.0 * fwd).expand(500, 3).contiguous()  # all behind camera
    g = H.gpu_forward(inp)
    o = H.oracle_forward(inp)
    assert g[0] == 0 == o[0]
    np.testing.assert_array_equal(g[1].cpu().numpy(), o[1])
    grads = H.upstream_grads(96, 128, 0)
    gb = H.gpu_backward(inp, g, grads)
    for a in gb:
        assert not np.any(a)


def test_single_gaussian_known_answer():
    """Closed form: isotropic s=0.05 at z=2, f=32, 32x32 image:
    radius 4, centre (15.5, 15.5), conic (1/0.94, 0, 1/0.94)."""
    from dynamic3dgaussians_amd.camera import setup_camera
    cam = setup_camera(32, 32, np.array([[32, 0, 16], [0, 32, 16], [0, 0, 1.0]]), np.eye(4))
    inp = dict(bg=torch.zeros(3), means3D=torch.tensor([[0.0, 0.0, 2.0]]),
               colors=torch.tensor([[1.0, 0.5, 0.25]]), semantic_feature=None,
               opacity=torch.tensor([[0.8]]), scales=torch.full((1, 3), 0.05),
               rotations=torch.tensor([[1.0, 0, 0, 0]]), scale_modifier=1.0, cov3D_precomp=None,
               viewmatrix=torch.from_numpy(cam.viewmatrix.copy()),
               projmatrix=torch.from_numpy(cam.projmatrix.copy()), c_x=16.0, c_y=16.0,
               tan_fovx=cam.tanfovx, tan_fovy=cam.tanfovy, image_height=32, image_width=32,
               sh=None, degree=0, campos=torch.from_numpy(cam.campos.copy()))
    g = H.gpu_forward(inp)
    assert g[5].item() == 4 and g[0] == 4
    st = H.export_state(1, 32, 32, g)
    np.testing.assert_allclose(st["means2D"][0], [15.5, 15.5])
    np.testing.assert_allclose(st["conic_opacity"][0, :3], [1 / 0.94, 0, 1 / 0.94], rtol=1e-6)
    a = 0.8 * np.exp(-0.5 * (0.25 + 0.25) / 0.94)
    np.testing.assert_allclose(g[1][:, 15, 15].cpu().numpy(), a * np.array([1, 0.5, 0.25]), rtol=1e-6)


def test_huge_gaussian_and_odd_sizes():
    inp = H.scene(P=50, W=37, H=29, scale_mult=40.0)
    _cmp_forward(inp, "fixed", 0)


def test_mark_visible():
    from dynamic3dgaussians_amd import _C
    inp = H.scene(P=5000)
    m = inp["means3D"].clone()
    m[::3, 2] += 5.0
    vis = _C.mark_visible(m.cuda(), inp["viewmatrix"].cuda(), inp["projmatrix"].cuda())
    ref = O.mark_visible(m, inp["viewmatrix"], inp["projmatrix"])
    np.testing.assert_array_equal(vis.cpu().numpy(), ref)


def test_prefiltered_error():
    inp = H.scene(P=100)
    inp["means3D"][0] = inp["campos"] - 2.0 * inp["viewmatrix"][:3, 2]  # behind the camera
    args = H.fwd_args(inp, "cuda")
    args[-2] = True  # prefiltered
    with pytest.raises(_lib.GsplatError, match="prefiltered"):
        from dynamic3dgaussians_amd import _C
        _C.rasterize_gaussians(*args)


# ------------------------------------------------------- fused label mask (Q12)

@pytest.mark.parametrize("use_sh", [False, True])
def test_fused_label_mask_matches_wrapper_mask(use_sh):
    """The label mask fused into preprocess_bwd equals the reference
    wrapper's `grad * label.unsqueeze(1)` (__init__.py:159-173): a single fp32
    multiply of the same value, so bit-identical up to backward's atomic order."""
    inp = H.scene(F=32, use_sh=use_sh, sh_degree=2 if use_sh else 0)
    P = inp["means3D"].size(0)
    g = torch.Generator().manual_seed(3)
    label = (torch.rand(P, generator=g) > 0.3).float() * torch.rand(P, generator=g).add(0.5)
    fwd = H.gpu_forward(inp)
    grads = H.upstream_grads(inp["image_height"], inp["image_width"], 32)
    plain = H.gpu_backward(inp, fwd, grads)
    num_rendered, color, feat, depth, alpha, radii, geom, binning, img = fwd
    dc, df, dd, da = [t.to(H.DEV) for t in grads]
    d = lambda k: H._to(inp[k], H.DEV)  # noqa: E731
    fused = _C.rasterize_gaussians_backward(
        d("bg"), d("means3D"), radii, d("colors"), d("semantic_feature"), d("scales"),
        d("rotations"), 1.0, d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"),
        *H.bwd_cam4(inp, True), dc, df, dd, da, d("sh"), inp["degree"], d("campos"), geom,
        num_rendered, binning, img, alpha, False, grad_mask=label.to(H.DEV))
    fused = [t.cpu() for t in fused]
    # The two backward runs differ only by fp32 atomic ordering, so compare at
    # that tolerance; rows with label 0 must be exactly zero.
    zero = label == 0
    for i, name in enumerate(GRAD_NAMES):
        ref = torch.from_numpy(plain[i])
        if name not in ("dmeans2D", "dsemantic"):
            ref = ref * (label[:, None, None] if ref.dim() == 3 else label[:, None])
            assert torch.count_nonzero(fused[i][zero]).item() == 0, name
        if torch.count_nonzero(ref).item():
            assert H.rel_l2(fused[i].numpy(), ref.numpy()) <= 1e-5, name
        else:
            assert torch.count_nonzero(fused[i]).item() == 0, name


def test_reference_mode_alpha_is_zero():
    """Q1: out_alpha of the reference is never written -> zeros (the kernel
    stores them, so a recycled allocation cannot leak through)."""
    inp = H.scene(F=0)
    junk = torch.full((1, 96, 128), 7.0, device=H.DEV)  # dirty the caching allocator
    del junk
    assert H.gpu_forward(inp, "reference")[4].abs().sum().item() == 0
    a = H.gpu_forward(inp, "fixed")[4]
    assert a.max().item() > 0.5


def test_absent_upstream_gradients_are_zeros():
    """Unused outputs give None grads (no materialized zeros); the binding
    treats them as zero images -- same result as passing zeros."""
    inp = H.scene(F=8)
    g = H.gpu_forward(inp)
    z = H.upstream_grads(inp["image_height"], inp["image_width"], 8)
    dc, df, dd, da = z
    zeros = [dc, torch.zeros_like(df), dd, torch.zeros_like(da)]
    full = H.gpu_backward(inp, g, zeros)
    num_rendered, color, feat, depth, alpha, radii, geom, binning, img = g
    d = lambda k: H._to(inp[k], H.DEV)  # noqa: E731
    part = _C.rasterize_gaussians_backward(
        d("bg"), d("means3D"), radii, d("colors"), d("semantic_feature"), d("scales"),
        d("rotations"), 1.0, d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"),
        *H.bwd_cam4(inp, True), dc.to(H.DEV), None, dd.to(H.DEV), None, d("sh"), inp["degree"],
        d("campos"), geom, num_rendered, binning, img, alpha, False)
    for a, b in zip(full, part):
        b = b.cpu().numpy()
        assert a.shape == b.shape
        if a.size:
            assert H.rel_l2(b, a) <= 1e-5 or np.abs(a).max() == 0



@pytest.mark.parametrize("F,Fp", [(20, 32), (35, 36)])
def test_binding_pads_masks_and_accumulates_against_oracle(F, Fp):
    """Feature widths the binding pads (35 -> 36 takes the padded-stride feature
    gradient scratch), SH and a label mask against the CPU oracle: the forward
    at _cmp_forward's bars with F channels, the masked gradients within 1e-4;
    caller buffers (`out`) hold the returned gradients, twice with accumulate."""
    assert _C.native_loaded()
    inp = H.scene(P=3000, F=F, sh_degree=2, use_sh=True, W=96, H=80)
    grads = H.upstream_grads(80, 96, F)
    label = torch.from_numpy((np.arange(3000) % 3 != 0).astype(np.float32))
    f, o = _cmp_forward(inp, "reference", F)
    assert f[2].shape == (F, 80, 96)
    args = _backward_args(inp, f, grads)
    b = [t.cpu() for t in _C.rasterize_gaussians_backward(*args, grad_mask=label.to(H.DEV))]
    bufs = _C.backward_buffers(3000, Fp, inp["sh"].shape[1], H.DEV)
    same = _C.rasterize_gaussians_backward(*args, grad_mask=label.to(H.DEV), out=bufs)
    once = {k: v.cpu().numpy() for k, v in bufs.items()}
    _C.rasterize_gaussians_backward(*args, grad_mask=label.to(H.DEV), out=bufs, accumulate=True)
    torch.cuda.synchronize()
    for name, a, ref in zip(GRAD_NAMES, b, H.oracle_backward(inp, o, grads)):
        ref = torch.from_numpy(ref)
        assert a.shape == ref.shape, name
        if name not in ("dmeans2D", "dsemantic"):
            ref = ref * (label[:, None, None] if ref.dim() == 3 else label[:, None])
            assert torch.count_nonzero(a[label == 0]).item() == 0, name
        if torch.count_nonzero(ref).item():
            assert H.rel_l2(a.numpy(), ref.numpy()) <= 1e-4, (name, H.rel_l2(a.numpy(), ref.numpy()))
        else:
            assert not a.any() or a.abs().max() < 1e-6, name
    # the caller's buffers: the returned gradients up to the fp32 atomics' order, dsem at the compiled width
    assert b[2].shape == (3000, F) and same[2].shape == (3000, F) and bufs["dsem"].shape == (3000, Fp)
    assert not once["dsem"][:, F:].any()
    for k, a in zip(_C._BUFFER_ORDER, b):
        x = once[k][:, :F] if k == "dsem" else once[k]
        assert H.rel_l2(x, a.numpy()) <= 1e-5 or not (a.any() or x.any()), k
    # the accumulated buffers hold twice the single call's gradients
    assert H.rel_l2(bufs["dmeans3D"].cpu().numpy(), 2 * b[4].numpy()) <= 1e-5


def _backward_args(inp, fwd, grads):
    num_rendered, color, feat, depth, alpha, radii, geom, binning, img = fwd
    d = lambda k: H._to(inp[k], H.DEV)  # noqa: E731
    return (d("bg"), d("means3D"), radii, d("colors"), d("semantic_feature"), d("scales"), d("rotations"),
            inp["scale_modifier"], d("cov3D_precomp"), d("viewmatrix"), d("projmatrix"), *H.bwd_cam4(inp, True),
            *[t.to(H.DEV) for t in grads], d("sh"), inp["degree"], d("campos"), geom, num_rendered, binning, img,
            alpha, False)


def test_single_camera_abi_entry_points_match_the_binding():
    """gs_forward_plan / gs_forward_render / gs_backward -- the reference-shaped
    single-camera entry points of the C ABI, which the
    package itself reaches only as a batch of one -- driven with ctypes
    directly: outputs bit-equal to _C.rasterize_gaussians, gradients equal to
    _C.rasterize_gaussians_backward up to the atomic backward's summation
    order."""
    import ctypes
    P, F, W, Hh = 3000, 8, 96, 80
    inp = H.scene(P=P, F=F, W=W, H=Hh)
    grads = H.upstream_grads(Hh, W, F)
    ref_f = H.gpu_forward(inp)
    ref_b = H.gpu_backward(inp, ref_f, grads)

    L_ = _lib.load()
    t = {k: H._to(inp[k], H.DEV).float().contiguous() for k in (
        "bg", "means3D", "colors", "semantic_feature", "opacity", "scales", "rotations", "viewmatrix",
        "projmatrix", "campos")}
    assert t["semantic_feature"].numel() == P * F
    p = lambda x: x.data_ptr() if x.numel() else None  # noqa: E731
    g = _lib.GsGaussians(P=P, D=0, M=0, F=F, means3D=p(t["means3D"]), colors_precomp=p(t["colors"]),
                         semantic_feature=p(t["semantic_feature"]), opacities=p(t["opacity"]),
                         scales=p(t["scales"]), rotations=p(t["rotations"]), scale_modifier=1.0)

    def camera(c_x, c_y, tan_fovx, tan_fovy):
        return _lib.GsCamera(viewmatrix=p(t["viewmatrix"]), projmatrix=p(t["projmatrix"]), campos=p(t["campos"]),
                             background=p(t["bg"]), c_x=c_x, c_y=c_y, tan_fovx=tan_fovx, tan_fovy=tan_fovy,
                             image_width=W, image_height=Hh)
    dev = t["means3D"].device
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(max(1, n), dtype=torch.uint8, device=dev)  # noqa: E731
    color, feat, depth, alpha = f32(3, Hh, W), f32(F, Hh, W), f32(1, Hh, W), f32(1, Hh, W)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    geom, img = u8(L_.gs_geom_buffer_bytes(P)), u8(L_.gs_image_buffer_bytes(W, Hh))
    s = _lib.stream(dev)
    cam = camera(inp["c_x"], inp["c_y"], inp["tan_fovx"], inp["tan_fovy"])
    NR, NI = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(L_.gs_forward_plan(ctypes.byref(g), ctypes.byref(cam), 0, 0, 0, p(geom), p(img), p(radii),
                                  ctypes.byref(NR), ctypes.byref(NI), s), "gs_forward_plan")
    assert 0 < NI.value <= NR.value
    binning = u8(L_.gs_binning_buffer_bytes(NI.value))
    _lib.check(L_.gs_forward_render(ctypes.byref(g), ctypes.byref(cam), 0, 0, p(geom), p(binning), p(img), NI.value,
                                    p(radii), p(color), p(feat), p(depth), p(alpha), s), "gs_forward_render")
    torch.cuda.synchronize()
    assert NR.value == ref_f[0]
    for name, a, b in zip(("color", "feature_map", "depth", "alpha", "radii"), (color, feat, depth, alpha, radii),
                          ref_f[1:6]):
        assert a.shape == b.shape and torch.equal(a, b), name

    # the backward as the binding runs it in reference mode (Q2: swapped camera scalars)
    bcam = camera(*H.bwd_cam4(inp, True))
    dc, df, dd, da = [x.to(dev).contiguous() for x in grads]
    out = _C.backward_buffers(P, F, 0, dev)
    scratch = u8(L_.gs_backward_scratch_bytes(P, F))
    _lib.check(L_.gs_backward(ctypes.byref(g), ctypes.byref(bcam), p(radii), 0, 0, p(geom), p(binning), p(img),
                              NR.value, p(alpha), p(dc), p(df), p(dd), p(da), p(scratch),
                              *[p(out[k]) for k in _C._BUFFER_ORDER], s), "gs_backward")
    torch.cuda.synchronize()
    for k, b in zip(_C._BUFFER_ORDER, ref_b):
        a = out[k].cpu().numpy()
        assert a.shape == b.shape, k
        assert H.rel_l2(a, b) <= 1e-5 or (not a.any() and not b.any()), k


def test_backward_out_contract_is_checked_before_any_launch():
    """rasterize_gaussians_backward(out=...) takes the GradientSink contract
    only: every gradient name, each in its exact shape (a buffer of the right
    element count but another shape is refused), and accumulate=True needs
    `out`.  Each bad call raises before any launch: the buffers are untouched."""
    from dynamic3dgaussians_amd import _C as C
    P, F = 3000, 8
    inp = H.scene(P=P, F=F, W=96, H=80)
    args = _backward_args(inp, H.gpu_forward(inp), H.upstream_grads(80, 96, F))
    bufs = C.backward_buffers(P, F, 0, H.DEV)
    for v in bufs.values():
        v.fill_(7.0)
    assert C.native_loaded()
    reshaped = dict(bufs, dmeans3D=torch.full((3, P), 7.0, device=H.DEV))
    with pytest.raises(RuntimeError, match="dmeans3D"):
        C.rasterize_gaussians_backward(*args, out=reshaped)
    missing = {k: v for k, v in bufs.items() if k != "dcov3D"}
    with pytest.raises(RuntimeError, match="dcov3D"):
        C.rasterize_gaussians_backward(*args, out=missing)
    with pytest.raises(ValueError, match="accumulate=True needs"):
        C.rasterize_gaussians_backward(*args, out=None, accumulate=True)
    torch.cuda.synchronize()
    for k, v in {**bufs, "reshaped": reshaped["dmeans3D"]}.items():
        assert torch.equal(v, torch.full_like(v, 7.0)), k


def test_debug_mode_validates_and_passes_on_a_valid_scene():
    """debug=True: the forward checks its plan header, ranges and list ids on
    the host (gs_check_*, gsplat_hip.h) before the blend; a valid scene
    passes and renders exactly what the non-debug call renders."""
    inp = H.scene(P=3000, F=8)
    a = _C.rasterize_gaussians(*H.fwd_args(inp, H.DEV))
    args = H.fwd_args(inp, H.DEV)
    args[-1] = True  # debug
    b = _C.rasterize_gaussians(*args)
    torch.cuda.synchronize()
    assert a[0] == b[0]
    for x, y in zip(a[1:6], b[1:6]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("compat", ["reference", "fixed"])
def test_unnormalised_quaternions_q7(compat):
    """Q7 (CR/forward.cu:129-163 and backward.cu:295-358): the reference's
    kernels build the rotation from the RAW quaternion, without normalising
    it (its Python callers normalise first, helpers.py:102, but the kernel
    boundary does not).  Every other test scene feeds unit quaternions, where
    the raw and the normalised forms coincide; here |q| spans about
    0.6 .. 1.6, so the covariance, its 2D projection and the scale / rotation
    gradients are the raw-quaternion ones: preprocess records bit-exact vs the
    oracle, images at the forward bar, gradients <= 1e-4 relative L2."""
    inp = H.scene(P=3000, F=8)
    g = torch.Generator().manual_seed(17)
    f = torch.exp(0.2 * torch.randn(3000, 1, generator=g)).clamp(0.6, 1.6)
    inp["rotations"] = (inp["rotations"] * f).contiguous()
    gf, of = _cmp_forward(inp, compat, 8)
    P, W, Hh = 3000, inp["image_width"], inp["image_height"]
    st_g, st_o = H.export_state(P, W, Hh, gf), of[6]
    vis = st_o.radii > 0
    np.testing.assert_array_equal(st_g["conic_opacity"][vis], st_o.conic_opacity[vis])
    # the raw quaternion really changes the covariance (Q7 is exercised)
    unit = dict(inp, rotations=torch.nn.functional.normalize(inp["rotations"], dim=1))
    assert not np.array_equal(H.oracle_forward(unit, compat)[6].conic_opacity[vis], st_o.conic_opacity[vis])
    grads = H.upstream_grads(Hh, W, 8)
    gb = H.gpu_backward(inp, gf, grads, compat)
    ob = H.oracle_backward(inp, of, grads, compat)
    for name, a, b in zip(GRAD_NAMES, gb, ob):
        if b.size == 0 or not np.any(b):
            continue
        assert H.rel_l2(a, b) <= 1e-4, (name, H.rel_l2(a, b))


# ---------------------------------------------------------------- fp16 split ranges

@pytest.mark.parametrize("compat", ["reference", "fixed"])
@pytest.mark.parametrize("F", [32, 36])
def test_fp16_split_contractions_across_channel_ranges(compat, F):
    """The forward's feature contraction and the backward's weight
    contractions run on fp16 two-piece splits under power-of-two scales: per
    feature channel (forward, from the table's largest |feature|) and per
    upstream-gradient row (backward, per strip).  Channels and rows whose
    magnitudes differ by up to 1e12 -- a zero channel, 1e6 and 1e-6 channels,
    a channel mixing 1e4 and 1e-4 rows, colour / depth / feature gradients at
    1e-3 .. 1e5 and a zero gradient plane -- each hold the parity bar on their
    own scale: every forward feature plane and every backward feature-gradient
    channel within 1e-5 / 1e-4 relative of the oracle's."""
    inp = H.scene(P=3000, F=F)
    f = inp["semantic_feature"].clone()
    f[:, 0] = 0.0
    f[:, 1] *= 1e6
    f[:, 2] *= 1e-6
    f[::2, 3] *= 1e4
    f[1::2, 3] *= 1e-4
    inp["semantic_feature"] = f.contiguous()
    g = H.gpu_forward(inp, compat)
    o = H.oracle_forward(inp, compat)
    assert g[0] == o[0]
    fg, fo = g[2].cpu().numpy(), o[2]
    for ch in range(F):
        ref = fo[ch]
        if not np.any(ref):
            assert not np.any(fg[ch]), ch
            continue
        # per channel: its own magnitude (1e-5 relative of the plane's largest value,
        # the forward bar; one flipped alpha decision aside)
        bad = np.abs(fg[ch] - ref) > 1e-5 * np.abs(ref).max()
        assert bad.mean() <= 1e-3, (ch, bad.mean())
    dc, df, dd, da = H.upstream_grads(inp["image_height"], inp["image_width"], F)
    dc = dc * torch.tensor([1e-3, 1.0, 1e5]).view(3, 1, 1)
    dd = dd * 1e3
    df = df.clone()
    df[4] = 0.0
    df[5] *= 1e-8
    df[6] *= 1e5
    grads = (dc, df, dd, da)
    gb = H.gpu_backward(inp, g, grads, compat)
    ob = H.oracle_backward(inp, o, grads, compat)
    for name, a, b in zip(GRAD_NAMES, gb, ob):
        if b.size == 0 or not np.any(b):
            continue
        assert H.rel_l2(a, b) <= 1e-4, (name, H.rel_l2(a, b))
    ds_g, ds_o = gb[2], ob[2]
    for ch in range(F):
        if not np.any(ds_o[:, ch]):
            assert not np.any(ds_g[:, ch]), ch
            continue
        assert H.rel_l2(ds_g[:, ch], ds_o[:, ch]) <= 1e-4, (ch, H.rel_l2(ds_g[:, ch], ds_o[:, ch]))
    dc_g, dc_o = gb[1], ob[1]
    for ch in range(3):  # the colour rows' own scales (1e-3 .. 1e5 apart)
        assert H.rel_l2(dc_g[:, ch], dc_o[:, ch]) <= 1e-4, (ch, H.rel_l2(dc_g[:, ch], dc_o[:, ch]))
