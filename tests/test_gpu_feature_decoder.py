"""The fused 1x1 feature decoder + L1 loss (include/gs_feature_decoder.h) on the GPU against
the float64 twin on the CPU, never against the code under test.

Targets are decision-robust: target = fp32(y64 + e) with |e| uniform in [0.05, 1] and a random
sign, so the fp32 signs equal the float64 ones on every element; the tests assert that
|r64| > 16 E everywhere (kept share 1.0) before comparing.  Bounds, with u = 2^-24, derived and
not measured (n_t and n_acc are read from the library):

    forward            |y - y64| <= (F_in + 4) u (sum_f |W x| + |b|)                    per element
    E                  (F_in + 5) u (sum_f |W x| + |b| + |target|)                      per element
    loss               (sum m E + n_t u sum m |r64|) / N
    d_x, sign mode     (C_out + 4) u up/N m sum_c |W[c,f]| |s|
    d_x, upstream      (C_out + 4) u sum_c |W g|
    d_W, d_b           (n_acc + 4) u sum |s m x| up/N,  (n_acc + 4) u sum |s m| up/N
    d_W, d_b upstream  (n_acc + 4) u sum |g x|,         (n_acc + 4) u sum |g|

Each case prints its measured maximum as a fraction of its bound before asserting.  Measured on
an MI355X over all shapes (profiles/feature_decoder/parity.json), largest error / bound: forward
0.20, loss 0.052, d_x 0.23 (upstream 0.19), d_W 0.021 (upstream 0.024), d_b 0.018 (upstream 0.017).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (FeatureDecoder, bilinear_resize, decode_features, decode_features_torch,
                                    decoded_distillation_loss, decoded_l1_loss, decoded_l1_loss_torch,
                                    distillation_image_loss,
                                    feature_distillation_loss, photometric_image_loss, photometric_loss)
from dynamic3dgaussians_amd import _lib
from dynamic3dgaussians_amd._lib import GsplatError
from dynamic3dgaussians_amd.camera import camera_rig
from dynamic3dgaussians_amd.rasterizer import GaussianRasterizationSettings
from dynamic3dgaussians_amd.scene import make_gaussians
from dynamic3dgaussians_amd.timesteps import TimestepDriver, batch_renderer, params2rendervar

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 1, 7), (1, 32, 64, 37, 53), (2, 64, 128, 12, 31), (1, 20, 384, 9, 65),
          (1, 32, 512, 5, 9), (1, 64, 256, 5, 9), (3, 32, 64, 72, 128), (1, 8, 8, 288, 512)]


@functools.lru_cache(maxsize=None)
def _case(shape, with_bias):
    """Inputs (fp32, CPU) and everything of the float64 reference that does not depend on the mask."""
    B, F_in, C_out, h, w = shape
    gen = torch.Generator().manual_seed(1000 + sum(shape) + int(with_bias))
    x = torch.randn(B, F_in, h, w, generator=gen)
    W = torch.randn(C_out, F_in, generator=gen) / F_in ** 0.5
    b = torch.randn(C_out, generator=gen) if with_bias else None
    y64 = decode_features_torch(x.double(), W.double(), None if b is None else b.double())
    e = (0.05 + 0.95 * torch.rand(y64.shape, generator=gen, dtype=torch.float64))
    e = e * (torch.randint(0, 2, y64.shape, generator=gen) * 2 - 1)
    target = (y64 + e).float().contiguous()
    mags = torch.einsum("cf,bfhw->bchw", W.double().abs(), x.double().abs())
    if b is not None:
        mags = mags + b.double().abs()[None, :, None, None]
    masks = {"none": None, "hw": _mask((h, w), gen), "bhw": _mask((B, h, w), gen)}
    up = 0.5 + torch.rand(B, generator=gen)
    g = torch.randn(y64.shape, generator=gen)
    return dict(x=x, W=W, b=b, y64=y64, target=target, mags=mags, masks=masks, up=up, g=g)


def _mask(shape, gen):
    m = torch.rand(shape, generator=gen)
    return torch.where(torch.rand(shape, generator=gen) < 0.3, torch.zeros(()), m.clamp_min(1e-3))


def _dev(t):
    return None if t is None else t.to(DEV)


FRACTIONS = []  # (quantity, max error / bound) of every comparison made (tools/feature_decoder_bench.py --parity)


def _frac(name, got, want, bound):
    err = (got.detach().cpu().double() - want).abs()
    frac = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    worst = float((err - bound).max())
    print(f"{name}: max error / bound = {frac:.3f}")
    FRACTIONS.append((name, frac))
    assert worst <= 0.0, (name, frac)
    return frac


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_fp64_twin(shape, with_bias):
    B, F_in, C_out, h, w = shape
    c = _case(shape, with_bias)
    L = _lib.load()
    N = C_out * h * w
    n_t, n_acc = L.gs_feature_decoder_n_t(C_out), L.gs_feature_decoder_n_acc(B, h, w)
    assert n_t > 0 and n_acc > 0
    x64, W64 = c["x"].double(), c["W"].double()
    b64 = None if c["b"] is None else c["b"].double()

    # ---- plain decode, forward and the upstream-mode backward
    xd, Wd, bd = (_dev(c[k]) for k in ("x", "W", "b"))
    leaves = [t.requires_grad_() for t in (xd, Wd, bd) if t is not None]
    y = decode_features(xd, Wd, bd)
    _frac("forward", y, c["y64"], (F_in + 4) * U * c["mags"])
    grads = torch.autograd.grad(y, leaves, _dev(c["g"]))
    g64 = c["g"].double()
    want_dx = torch.einsum("cf,bchw->bfhw", W64, g64)
    _frac("d_x upstream", grads[0], want_dx,
          (C_out + 4) * U * torch.einsum("cf,bchw->bfhw", W64.abs(), g64.abs()))
    _frac("d_W upstream", grads[1], torch.einsum("bchw,bfhw->cf", g64, x64),
          (n_acc + 4) * U * torch.einsum("bchw,bfhw->cf", g64.abs(), x64.abs()))
    if bd is not None:
        _frac("d_b upstream", grads[2], g64.sum(dim=(0, 2, 3)), (n_acc + 4) * U * g64.abs().sum(dim=(0, 2, 3)))

    # ---- fused loss, three masks
    t64 = c["target"].double()
    r64 = c["y64"] - t64
    E = (F_in + 5) * U * (c["mags"] + t64.abs())
    assert bool((r64.abs() > 16 * E).all()), "the targets are not decision-robust: kept share < 1.0"
    s64 = torch.sign(r64)
    up64 = c["up"].double()
    td, upd = _dev(c["target"]), _dev(c["up"])
    for name, m in c["masks"].items():
        m64 = torch.ones(B, h, w, dtype=torch.float64) if m is None else m.double().expand(B, h, w)
        mb = m64[:, None]
        xd, Wd, bd = (_dev(c[k]) for k in ("x", "W", "b"))
        leaves = [t.requires_grad_() for t in (xd, Wd, bd) if t is not None]
        loss = decoded_l1_loss(xd, Wd, bd, td, mask=_dev(m), reduction="none")
        want = decoded_l1_loss_torch(x64, W64, b64, t64, mask=None if m is None else m.double(), reduction="none")
        _frac(f"loss[{name}]", loss, want,
              ((mb * E).sum(dim=(1, 2, 3)) + n_t * U * (mb * r64.abs()).sum(dim=(1, 2, 3))) / N)
        grads = torch.autograd.grad((loss * upd).sum(), leaves)
        sc = (up64 / N)[:, None, None, None]
        sm = s64 * mb * sc
        _frac(f"d_x[{name}]", grads[0], torch.einsum("cf,bchw->bfhw", W64, sm),
              (C_out + 4) * U * torch.einsum("cf,bchw->bfhw", W64.abs(), sm.abs()))
        _frac(f"d_W[{name}]", grads[1], torch.einsum("bchw,bfhw->cf", sm, x64),
              (n_acc + 4) * U * torch.einsum("bchw,bfhw->cf", sm.abs(), x64.abs()))
        if bd is not None:
            _frac(f"d_b[{name}]", grads[2], sm.sum(dim=(0, 2, 3)), (n_acc + 4) * U * sm.abs().sum(dim=(0, 2, 3)))
        # reduction="sum" is the sum over the cameras
        assert decoded_l1_loss(xd, Wd, bd, td, mask=_dev(m)).item() == loss.sum().item()


@pytest.mark.parametrize("shape", [(1, 64, 96, 3, 50), (1, 20, 33, 2, 37)], ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_data_is_reproduced_bit_for_bit(shape):
    """Asymmetric small-integer operands: every product and sum is exact, so a row/column swap, a
    wrong k permutation or a wrong transpose changes the result outright."""
    B, F_in, C_out, h, w = shape
    P = h * w
    N = C_out * P
    ci, fi, pi = torch.arange(C_out), torch.arange(F_in), torch.arange(P)
    W = (((3 * ci[:, None] + 5 * fi[None, :]) % 17) - 8).double()
    x = (((7 * fi[:, None] + 11 * pi[None, :]) % 13) - 6).double().reshape(1, F_in, h, w)
    b = (ci % 5).double()
    y = torch.einsum("cf,bfhw->bchw", W, x) + b[None, :, None, None]
    r = (((ci[:, None] + 2 * pi[None, :]) % 3) - 1).double().reshape(1, C_out, h, w)
    target = y - r  # y - target = r in {-1, 0, +1}
    s = torch.sign(r)
    assert float(y.abs().max()) < 2 ** 24 and bool((s == 0).any())
    want = dict(dx=torch.einsum("cf,bchw->bfhw", W, s), dW=torch.einsum("bchw,bfhw->cf", s, x),
                db=s.sum(dim=(0, 2, 3)))

    def leaves():
        return [t.float().to(DEV).requires_grad_() for t in (x, W, b)]

    xd, Wd, bd = leaves()
    yd = decode_features(xd, Wd, bd)
    assert torch.equal(yd.cpu().double(), y)
    for mode in ("sign", "upstream"):
        xd, Wd, bd = leaves()
        if mode == "sign":
            loss = decoded_l1_loss(xd, Wd, bd, target.float().to(DEV), reduction="none")
            total = float(r.abs().sum())
            assert loss.item() == float(np.float32(total / N)) and round(loss.item() * N) == total
            grads = torch.autograd.grad((loss * float(N)).sum(), (xd, Wd, bd))
        else:
            grads = torch.autograd.grad(decode_features(xd, Wd, bd), (xd, Wd, bd), s.float().to(DEV))
        for got, key in zip(grads, ("dx", "dW", "db")):
            assert torch.equal(got.cpu().double(), want[key]), (mode, key)


BIG = (3, 32, 64, 72, 128)


def _big_inputs(requires_grad=True):
    c = _case(BIG, True)
    out = [_dev(c[k]) for k in ("x", "W", "b")]
    if requires_grad:
        out = [t.requires_grad_() for t in out]
    return out + [_dev(c["target"]), _dev(c["masks"]["bhw"])]


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        xd, Wd, bd, td, md = _big_inputs()
        loss = decoded_l1_loss(xd, Wd, bd, td, mask=md, reduction="none")
        runs.append((loss.detach(),) + torch.autograd.grad(loss.sum(), (xd, Wd, bd)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_decoded_map_behind_the_fused_path():
    B, F_in, C_out, h, w = BIG
    L = _lib.load()
    xd, Wd, bd, td, md = _big_inputs()
    decoded_l1_loss(xd, Wd, bd, td, mask=md).backward()  # warm: library loaded, allocator primed
    xd.grad = Wd.grad = bd.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    decoded_l1_loss(xd, Wd, bd, td, mask=md).backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    ws = sum(L.gs_feature_decoder_workspace_bytes(B, F_in, C_out, h, w, p)
             for p in (_lib.FD_PASS_LOSS, _lib.FD_PASS_LOSS_BACKWARD))
    allowed = 4 * (xd.numel() + Wd.numel() + bd.numel()) + ws + (1 << 20)
    one_map = 4 * B * C_out * h * w
    print(f"peak over the inputs {extra} B, allowed {allowed} B, one decoded map {one_map} B")
    assert extra <= allowed
    assert allowed < one_map  # only if the slabs are sized by the grid and not by the pixels


# ---------------------------------------------------------------- wiring

def _wiring_inputs():
    gen = torch.Generator().manual_seed(77)
    feat = torch.randn(2, 32, 75, 130, generator=gen).to(DEV)
    target = torch.randn(2, 64, 48, 47, generator=gen).to(DEV)
    torch.manual_seed(5)
    dec = FeatureDecoder(32, 64).to(DEV)
    return feat, target, dec


def test_feature_distillation_loss_with_a_decoder_is_the_composition_bit_for_bit():
    feat, target, dec = _wiring_inputs()
    W, b = dec.conv.weight, dec.conv.bias
    resized = bilinear_resize(feat, (48, 47), align_corners=True)
    with torch.no_grad():
        assert torch.equal(decoded_distillation_loss(feat, target, dec),
                           decoded_l1_loss(resized, W, b, target))
        assert torch.equal(decoded_distillation_loss(feat, target, (W, b)),
                           decoded_l1_loss(resized, W, b, target))
        assert torch.equal(decoded_distillation_loss(feat, target, dec, l1_weight=0.8, ssim_weight=0.2),
                           photometric_loss(decode_features(resized, W, b), target, l1_weight=0.8, ssim_weight=0.2))
        # decoder=None: the parent's composition, same channel count on both sides
        t32 = target[:, :32].contiguous()
        assert torch.equal(feature_distillation_loss(feat, t32),
                           photometric_loss(resized, t32, l1_weight=1.0, ssim_weight=0.0))
    f = feat.clone().requires_grad_()
    decoded_distillation_loss(f, target, dec).backward()
    assert float(f.grad.abs().sum()) > 0 and float(dec.conv.weight.grad.abs().sum()) > 0


N_CAMS, WW, HH, P, NF = 4, 64, 48, 600, 32


def _settings():
    return [GaussianRasterizationSettings(
        image_height=HH, image_width=WW, tanfovx=c.tanfovx, tanfovy=c.tanfovy, c_x=c.c_x, c_y=c.c_y,
        bg=torch.zeros(3, device=DEV), viewmatrix=torch.from_numpy(c.viewmatrix.copy()).to(DEV),
        projmatrix=torch.from_numpy(c.projmatrix.copy()).to(DEV), sh_degree=0,
        campos=torch.from_numpy(c.campos.copy()).to(DEV)) for c in camera_rig(N_CAMS, WW, HH, seed=3)]


def _leaves():
    g = make_gaussians(P, F=NF, seed=4, scale_mult=3.0, device=DEV)
    p = {"means3D": g["means3D"], "rgb_colors": g["colors"], "unnorm_rotations": g["rotations"],
         "logit_opacities": torch.logit(g["opacities"].clamp(1e-4, 1 - 1e-4)), "log_scales": torch.log(g["scales"]),
         "semantic_feature": g["semantic_feature"]}
    return {k: torch.nn.Parameter(v.detach().clone().contiguous()) for k, v in p.items()}


def test_driver_step_with_a_decoder():
    """One TimestepDriver step with distillation_image_loss(decoder=dec) on a 4-camera render
    (F = 32, 64 x 48) against a 64-channel prior of 24 x 32, a torch Adam on the decoder."""
    settings = _settings()
    gen = torch.Generator().manual_seed(12)
    tg = torch.rand(N_CAMS, 3, HH, WW, generator=gen).to(DEV)
    prior = torch.randn(N_CAMS, 2 * NF, 24, 32, generator=gen).to(DEV)
    torch.manual_seed(6)
    dec = FeatureDecoder(NF, 2 * NF).to(DEV)
    W0, b0 = dec.conv.weight.detach().clone(), dec.conv.bias.detach().clone()
    dec_opt = torch.optim.Adam(dec.parameters(), lr=1e-3)
    params = _leaves()
    opt = torch.optim.SGD([{"params": [params[k]], "name": k, "lr": 0.0} for k in params], lr=0.0)
    drv = TimestepDriver(params, {}, opt, N_CAMS, batch_renderer(settings),
                         image_loss=functools.partial(distillation_image_loss, feature_weight=1.0, decoder=dec))
    loss = float(drv.step((tg, prior)))
    assert np.isfinite(loss)
    gW, gb = dec.conv.weight.grad, dec.conv.bias.grad
    assert gW is not None and float(gW.abs().sum()) > 0 and float(gb.abs().sum()) > 0
    assert float(params["semantic_feature"].grad.abs().sum()) > 0
    dec_opt.step()
    assert not torch.equal(dec.conv.weight.detach(), W0)

    # the same render, the feature term by the float64 twin
    with torch.no_grad():
        (im, feat), _stats = batch_renderer(settings)(params2rendervar(_leaves()), list(range(N_CAMS)))
        colour = float(photometric_image_loss(im, tg))
        resized = bilinear_resize(feat.contiguous(), (24, 32), align_corners=True).cpu().double()
    W64, b64, t64 = W0.reshape(2 * NF, NF).cpu().double(), b0.cpu().double(), prior.cpu().double()
    want_f = decoded_l1_loss_torch(resized, W64, b64, t64, reduction="none")
    y64 = decode_features_torch(resized, W64, b64)
    mags = torch.einsum("cf,bfhw->bchw", W64.abs(), resized.abs()) + b64.abs()[None, :, None, None]
    E = (NF + 5) * U * (mags + t64.abs())
    n_t = _lib.load().gs_feature_decoder_n_t(2 * NF)
    bound = float(((E.sum(dim=(1, 2, 3)) + n_t * U * (y64 - t64).abs().sum(dim=(1, 2, 3))) / y64[0].numel()).sum())
    want = (colour + float(want_f.sum())) / N_CAMS
    err = abs(loss - want)
    allowed = bound / N_CAMS + 8 * U * abs(want)  # the fp32 sums of the two terms and the division
    print(f"driver loss {loss:.9g}, twin {want:.9g}: error / bound = {err / allowed:.3f}")
    assert err <= allowed


def test_errors():
    c = _case((2, 3, 5, 1, 7), True)
    x, W, b, t = (_dev(c[k]) for k in ("x", "W", "b", "target"))
    with pytest.raises(GsplatError, match="_torch"):
        decoded_l1_loss(c["x"], c["W"], c["b"], c["target"])
    with pytest.raises(GsplatError, match="_torch"):
        decode_features(c["x"], c["W"], c["b"])
    strided = torch.randn(2, 3, 7, 4, device=DEV).transpose(2, 3)[:, :, :1]  # [2, 3, 1, 7], not contiguous
    with pytest.raises(GsplatError, match="contiguous"):
        decoded_l1_loss(strided, W, b, t)
    with pytest.raises(GsplatError, match="16384"):
        decode_features(torch.zeros(1, 64, 2, 2, device=DEV), torch.zeros(257, 64, device=DEV))
    with pytest.raises(GsplatError, match="gradient"):
        decoded_l1_loss(x, W, b, t.clone().requires_grad_())
