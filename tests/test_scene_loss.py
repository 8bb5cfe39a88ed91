"""CPU tests of the scene regularisers and the foreground split (no GPU needed):
  * regularizer_losses_torch in fp64 reproduces the reference's losses and gradients (fixture
    tests/golden/scene_loss.npz, recorded from the statements of the reference's
    train.py:275-282 by tests/golden/make_golden_scene_loss.py), the NaN of an empty background
    included;
  * foreground_split gives the slot table of a numpy restatement, and its cache is dropped by
    an in-place edit and by a new mask object;
  * the library exports every symbol include/gs_scene_loss.h declares, each with a ctypes
    prototype, and the ctypes mirror of gs_scene_loss has the library's size and the header's
    fields; GS_ABI_VERSION is unchanged;
  * the host validator refuses every bad argument block with a message naming the field, and
    the wrappers refuse what the kernels cannot take (no CPU fallback);
  * the validator runs clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/scene_loss_host_sanitize.c);
  * reference_extra_loss: None at t == 0 and before the graph exists, its weights, and through
    TimestepDriver the hand-assembled sum (the three HIP calls replaced by torch restatements:
    the callable itself needs the device library).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import (_lib, foreground_split, gather_foreground, reference_extra_loss,
                                    regularizer_losses, regularizer_losses_torch, scene_loss)
from dynamic3dgaussians_amd.timesteps import TimestepDriver, l1_image_loss, params2rendervar
from tests._harness import run_host_sanitizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "scene_loss.npz")
CASES = ("tiny", "mixed", "all_fg")
TABLES = ("means3D", "rotations", "rgb_colors")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 100 * 1024
    sizes = {"tiny": (7, 3), "mixed": (1000, None), "all_fg": (5, 5)}
    for name in CASES:
        P, n_fg = sizes[name]
        fg = gold[f"{name}.is_fg"]
        assert fg.dtype == np.bool_ and fg.shape == (P,)
        n_fg = int(fg.sum()) if n_fg is None else n_fg
        assert int(fg.sum()) == n_fg
        for k, w in (("means3D", 3), ("rotations", 4), ("rgb_colors", 3), ("prev_col", 3)):
            assert gold[f"{name}.{k}"].shape == (P, w) and gold[f"{name}.{k}"].dtype == np.float32
            if k != "prev_col":
                assert gold[f"{name}.grad_{k}"].shape == (P, w) and gold[f"{name}.grad_{k}"].dtype == np.float64
        assert gold[f"{name}.init_bg_pts"].shape == (P - n_fg, 3) and gold[f"{name}.init_bg_rot"].shape == (P - n_fg, 4)
        assert gold[f"{name}.losses"].shape == (3,) and gold[f"{name}.up"].tolist() == [0.7, -1.3, 2.1]
    assert 0.35 < gold["mixed.is_fg"].mean() < 0.45
    # the kinks of `tiny`
    fg, m = gold["tiny.is_fg"], gold["tiny.means3D"]
    assert fg.tolist() == [True, False, True, False, False, True, False]
    assert m[0, 1] == 0.0 and m[2, 1] < 0 and m[5, 1] > 0
    assert m[3, 2] == gold["tiny.init_bg_pts"][1, 2]
    assert gold["tiny.rgb_colors"][4, 0] == gold["tiny.prev_col"][4, 0]
    # and what the reference's autograd made of them
    up = gold["tiny.up"]
    g = gold["tiny.grad_means3D"]
    assert g[0, 1] == up[0] / 3 and g[2, 1] == 0.0 and g[5, 1] == up[0] / 3   # clamp passes at y == 0
    assert g[3, 2] == 0.0 and abs(g[3, 0]) == abs(up[1]) / 4                   # abs: 0 at 0
    assert gold["tiny.grad_rgb_colors"][4, 0] == 0.0
    # an empty background: NaN loss, zero gradients behind it
    assert np.isnan(gold["all_fg.losses"][1]) and np.isfinite(gold["all_fg.losses"][[0, 2]]).all()
    assert not gold["all_fg.grad_rotations"].any() and np.isfinite(gold["all_fg.grad_means3D"]).all()


def _inputs(gold, name, dtype=torch.float64):
    t = lambda k: torch.from_numpy(gold[f"{name}.{k}"])  # noqa: E731
    tables = [t(k).to(dtype).requires_grad_(True) for k in TABLES]
    variables = {k: t(k).to(dtype) for k in ("init_bg_pts", "init_bg_rot", "prev_col")}
    return tables, variables, t("is_fg")


@pytest.mark.parametrize("as_split", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference_in_fp64(gold, name, as_split):
    """Both sides are fp64 torch on the CPU running the same operations: 1e-12 leaves four orders
    over fp64 rounding and catches any change of formula, order or gate."""
    tables, variables, is_fg = _inputs(gold, name)
    losses = regularizer_losses_torch(*tables, variables, foreground_split(is_fg) if as_split else is_fg)
    want = gold[f"{name}.losses"]
    for got, ref in zip(losses, want):
        assert got.dim() == 0
        assert (np.isnan(ref) and torch.isnan(got)) or abs(got.item() - ref) <= 1e-12 * max(1.0, abs(ref))
    total = sum(float(u) * v for u, v in zip(gold[f"{name}.up"], losses))
    grads = torch.autograd.grad(total, tables)
    for k, g in zip(TABLES, grads):
        ref = gold[f"{name}.grad_{k}"]
        assert np.array_equal(np.isnan(g.numpy()), np.isnan(ref))
        assert _rel(np.nan_to_num(g.numpy()), np.nan_to_num(ref)) <= 1e-12, k
        assert np.array_equal(g.numpy() == 0, ref == 0), k  # the kinks, element for element


def test_raw_rotations_restatement_normalises_first(gold):
    tables, variables, is_fg = _inputs(gold, "mixed")
    unit = torch.nn.functional.normalize(tables[1].detach())  # the fixture's rows are unit to fp32 only
    raw = (unit * (0.5 + torch.rand(1000, 1, dtype=torch.float64))).requires_grad_(True)
    a = regularizer_losses_torch(tables[0], raw, tables[2], variables, is_fg, raw_rotations=True)
    b = regularizer_losses_torch(tables[0], unit, tables[2], variables, is_fg)
    assert abs(a[1].item() - b[1].item()) <= 1e-12 and a[0] == b[0] and a[2] == b[2]
    (g,) = torch.autograd.grad(a[1], raw)
    assert (g * raw.detach()).sum(dim=1).abs().max() < 1e-15  # normalize's gradient is tangent to the sphere


# ------------------------------------------------------------ the split

def _slot_numpy(mask):
    """The slot table by its definition: ranks in the order of np.flatnonzero."""
    slot = np.empty(len(mask), np.int32)
    slot[np.flatnonzero(mask)] = np.arange(int(mask.sum()), dtype=np.int32)
    slot[np.flatnonzero(~mask)] = -1 - np.arange(int((~mask).sum()), dtype=np.int32)
    return slot


@pytest.mark.parametrize("P,frac", [(1, 0.0), (1, 1.0), (7, 0.4), (64, 0.0), (65, 1.0), (1000, 0.4), (4099, 0.9)])
def test_foreground_split_matches_numpy(P, frac):
    gen = torch.Generator().manual_seed(P)
    mask = torch.rand(P, generator=gen) < frac if 0.0 < frac < 1.0 else torch.full((P,), frac == 1.0)
    s = foreground_split(mask)
    assert s.slot.dtype == torch.int32 and s.slot.shape == (P,) and s.slot.is_contiguous()
    assert isinstance(s.n_fg, int) and isinstance(s.n_bg, int)
    assert (s.n_fg, s.n_bg, s.P) == (int(mask.sum()), P - int(mask.sum()), P)
    assert np.array_equal(s.slot.numpy(), _slot_numpy(mask.numpy()))
    # slot r addresses row r of x[is_fg] / x[~is_fg]
    assert torch.equal(s.slot[mask].long(), torch.arange(s.n_fg))
    assert torch.equal((-1 - s.slot[~mask]).long(), torch.arange(s.n_bg))


def test_foreground_split_takes_both_reference_forms_and_refuses_the_rest():
    seg = torch.tensor([[0.9, 0, 0], [0.1, 0, 0], [0.6, 0, 0]])
    label = torch.tensor([1, 0, 1])
    a, b = foreground_split(seg[:, 0] > 0.5), foreground_split(label == 1)
    assert a.slot.tolist() == b.slot.tolist() == [0, -1, 1]
    for bad in (torch.tensor([1, 0, 1]), torch.ones(2, 2, dtype=torch.bool), [True, False]):
        with pytest.raises(_lib.GsplatError, match="bool"):
            foreground_split(bad)


def test_split_cache_is_keyed_by_the_mask_object_and_its_version():
    variables = {}
    mask = torch.tensor([True, False, True, False])
    a = foreground_split(mask, variables)
    assert foreground_split(mask, variables) is a                      # a hit
    assert foreground_split(mask) is not a                             # no dict, no cache
    mask[1] = True                                                     # an in-place edit bumps _version
    b = foreground_split(mask, variables)
    assert b is not a and (b.n_fg, b.slot.tolist()) == (3, [0, 1, 2, -1])
    assert foreground_split(mask, variables) is b
    twin = mask.clone()                                                # equal values, another object
    c = foreground_split(twin, variables)
    assert c is not b and c.slot.tolist() == b.slot.tolist()
    assert foreground_split(mask, variables) is not c                  # one entry: the older mask is built again
    view = twin[:]                                                     # a view is another object too
    assert foreground_split(view, variables) is not c


# ------------------------------------------------------------ the C boundary

def _header():
    txt = open(os.path.join(REPO, "include", "gs_scene_loss.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


NAMES = ["gs_fg_gather_backward", "gs_fg_gather_forward", "gs_scene_loss_backward", "gs_scene_loss_forward",
         "gs_scene_loss_struct_bytes", "gs_scene_loss_validate", "gs_scene_loss_workspace_bytes"]


def test_library_exports_every_symbol_of_gs_scene_loss_h():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header())))
    assert names == NAMES
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 13 and _lib.load().gs_version() == 13  # a new header, no existing struct changed
    txt = open(os.path.join(REPO, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define\s+GS_ABI_VERSION\s+13\b", txt)


def _header_struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        names += [re.findall(r"[A-Za-z_]\w*", part)[-1] for part in decl.split(",")]
    return names


def test_ctypes_struct_mirrors_the_header():
    L = _lib.load()
    fields = [f for f, _ in _lib.GsSceneLoss._fields_]
    assert fields == _header_struct_fields("gs_scene_loss")
    assert fields == ["P", "n_fg", "n_bg", "slot", "means", "rotations", "colors", "init_bg_pts", "init_bg_rot",
                      "prev_col", "raw_rotations", "_pad", "losses", "workspace", "workspace_bytes"]
    assert ctypes.sizeof(_lib.GsSceneLoss) == L.gs_scene_loss_struct_bytes()


GRID_CAP = 8 * 256  # workgroups: csrc/gs_scene_loss_layout.h SL_MAX_GROUPS


def test_workspace_bytes():
    ws = _lib.load().gs_scene_loss_workspace_bytes
    assert ws(1) == 16 and ws(256) == 16 and ws(257) == 32            # one 4-float record per workgroup of 256 rows
    assert ws(300_000) == 1172 * 16
    assert ws(GRID_CAP * 256) == GRID_CAP * 16 == ws(GRID_CAP * 256 + 1) == ws(1 << 30)  # capped
    assert ws(0) == 0 and ws(-3) == 0


def _good_block(keep, P=10, n_fg=4):
    """A valid argument block over host arrays (the validator dereferences nothing)."""
    L = _lib.load()
    ws_bytes = L.gs_scene_loss_workspace_bytes(P)
    bufs = {k: np.zeros(P * 4 + 4, np.float32) for k in ("means", "rot", "col", "prev_col", "bg_pts", "bg_rot",
                                                         "d_means", "d_rot", "d_col")}
    bufs["slot"] = np.zeros(P + 1, np.int32)
    bufs["losses"], bufs["up"] = np.zeros(4, np.float32), np.zeros(4, np.float32)
    bufs["ws"] = np.zeros(ws_bytes // 4 + 64, np.float32)
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    a = _lib.GsSceneLoss(P=P, n_fg=n_fg, n_bg=P - n_fg, slot=p["slot"], means=p["means"], rotations=p["rot"],
                         colors=p["col"], init_bg_pts=p["bg_pts"], init_bg_rot=p["bg_rot"], prev_col=p["prev_col"],
                         losses=p["losses"], workspace=p["ws"], workspace_bytes=ws_bytes)
    return a, p


def test_validator_rejects_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    v = lambda a, bwd=0, up=None, dm=None, dr=None, dc=None: L.gs_scene_loss_validate(  # noqa: E731
        ctypes.byref(a), bwd, up, dm, dr, dc)
    a, p = _good_block(keep)
    grads = (p["up"], p["d_means"], p["d_rot"], p["d_col"])
    assert v(a) == 0 and v(a, 1, *grads) == 0
    a.rotations, a.raw_rotations = p["rot"] + 4, 1  # 4 bytes past a 16-byte boundary: the scalar path
    assert v(a) == 0
    a.losses, a.workspace, a.workspace_bytes = None, None, 0  # the backward needs neither
    assert v(a, 1, *grads) == 0
    a, _ = _good_block(keep, n_fg=10)
    a.init_bg_pts, a.init_bg_rot = None, None  # no background rows, no anchors
    assert v(a) == 0
    assert L.gs_scene_loss_validate(None, 0, None, None, None, None) < 0 and b"null argument" in L.gs_last_error()
    tables = b"means, rotations and colors are required"
    for field, value, msg in [("P", 0, b"P must be in"), ("P", -10, b"P must be in"), ("P", 1 << 31, b"P must be in"),
                              ("n_fg", -1, b"n_fg and n_bg must be >= 0"), ("n_bg", -6, b"n_fg and n_bg must be >= 0"),
                              ("n_fg", 5, b"n_fg + n_bg must equal P"), ("n_bg", 5, b"n_fg + n_bg must equal P"),
                              ("P", 11, b"n_fg + n_bg must equal P"),
                              ("slot", None, b"slot is required"), ("means", None, tables),
                              ("rotations", None, tables), ("colors", None, tables),
                              ("prev_col", None, b"prev_col is required"),
                              ("init_bg_pts", None, b"init_bg_pts and init_bg_rot are required"),
                              ("init_bg_rot", None, b"init_bg_pts and init_bg_rot are required"),
                              ("means", p["means"] + 2, b"every table must be 4-byte aligned"),
                              ("init_bg_rot", p["bg_rot"] + 1, b"every table must be 4-byte aligned"),
                              ("slot", p["slot"] + 3, b"every table must be 4-byte aligned"),
                              ("losses", None, b"losses is required"),
                              ("losses", p["losses"] + 1, b"losses must be 4-byte aligned"),
                              ("workspace", None, b"workspace is required"), ("workspace_bytes", 15, b"needed"),
                              ("workspace", p["ws"] + 4, b"16-byte aligned")]:
        bad, _ = _good_block(keep)
        setattr(bad, field, value)
        assert v(bad) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())
    a, p = _good_block(keep)
    up, dm, dr, dc = p["up"], p["d_means"], p["d_rot"], p["d_col"]
    assert v(a, 1, None, dm, dr, dc) < 0 and b"dL_dlosses is required" in L.gs_last_error()
    for miss in ((up, None, dr, dc), (up, dm, None, dc), (up, dm, dr, None)):
        assert v(a, 1, *miss) < 0 and b"dL_dmeans, dL_drotations and dL_dcolors are required" in L.gs_last_error()
    assert v(a, 1, up, dm, dr + 2, dc) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    assert v(a, 1, up + 1, dm, dr, dc) < 0 and b"gradient pointers must be 4-byte aligned" in L.gs_last_error()
    # the entry points run the validator before anything touches a device
    bad, _ = _good_block(keep)
    bad.n_fg = 3
    assert L.gs_scene_loss_forward(ctypes.byref(bad), None) < 0 and b"must equal P" in L.gs_last_error()
    assert L.gs_scene_loss_backward(ctypes.byref(bad), up, dm, dr, dc, None) < 0
    # and so do the gather's
    gf, gb = L.gs_fg_gather_forward, L.gs_fg_gather_backward
    assert gf(0, 0, p["slot"], p["means"], p["rot"], dm, dr, None) < 0 and b"P must be in" in L.gs_last_error()
    assert gf(10, 11, p["slot"], p["means"], p["rot"], dm, dr, None) < 0 and b"n_fg must be in" in L.gs_last_error()
    assert gf(10, -1, p["slot"], p["means"], p["rot"], dm, dr, None) < 0 and b"n_fg must be in" in L.gs_last_error()
    assert gf(10, 4, None, p["means"], p["rot"], dm, dr, None) < 0 and b"slot is required" in L.gs_last_error()
    assert gf(10, 4, p["slot"], None, p["rot"], dm, dr, None) < 0 and b"[P] tables are required" in L.gs_last_error()
    assert gf(10, 4, p["slot"], p["means"], p["rot"], None, dr, None) < 0 \
        and b"[n_fg] tables are required" in L.gs_last_error()
    assert gf(10, 4, p["slot"], p["means"] + 1, p["rot"], dm, dr, None) < 0 and b"4-byte aligned" in L.gs_last_error()
    assert gb(10, 4, None, dm, dr, dm, dr, None) < 0 and b"slot is required" in L.gs_last_error()
    assert gb(10, 4, p["slot"], dm, dr, dm + 2, dr, None) < 0 and b"4-byte aligned" in L.gs_last_error()
    assert gb(1 << 31, 4, p["slot"], dm, dr, dm, dr, None) < 0 and b"P must be in" in L.gs_last_error()


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrappers' dtype / layout / shape rules (all checked
    before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def test_wrappers_reject_what_the_kernels_cannot_take(gold):
    (m, q, c), variables, is_fg = _inputs(gold, "tiny", torch.float32)
    m, q, c = m.detach(), q.detach(), c.detach()
    split = foreground_split(is_fg)
    D = _DeviceClaim
    dv = {k: D(x) for k, x in variables.items()}
    dsplit = scene_loss.ForegroundSplit(D(split.slot), split.n_fg, split.n_bg, is_fg)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        regularizer_losses(m, q, c, variables, split)  # no CPU fallback
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        gather_foreground(m, q, split)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        regularizer_losses(D(m), D(q), D(c), dv, split)  # the slot table too
    with pytest.raises(_lib.GsplatError, match="float32"):
        regularizer_losses(D(m.double()), D(q), D(c), dv, dsplit)
    with pytest.raises(_lib.GsplatError, match="shape"):
        regularizer_losses(D(m), D(q[:, :3]), D(c), dv, dsplit)
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        regularizer_losses(D(m), D(q), D(torch.rand(3, 7).t()), dv, dsplit)
    with pytest.raises(_lib.GsplatError, match="foreground_split"):
        regularizer_losses(D(m), D(q), D(c), dv, is_fg)
    with pytest.raises(_lib.GsplatError, match="the split is over 7 rows"):
        regularizer_losses(D(m[:5].clone()), D(q[:5].clone()), D(c[:5].clone()), dv, dsplit)
    with pytest.raises(_lib.GsplatError, match="init_bg_pts must have shape"):
        regularizer_losses(D(m), D(q), D(c), dict(dv, init_bg_pts=D(torch.zeros(3, 3))), dsplit)
    with pytest.raises(_lib.GsplatError, match="no gradient"):
        regularizer_losses(D(m), D(q), D(c), dict(dv, prev_col=D(variables["prev_col"].clone().requires_grad_(True))),
                           dsplit)
    with pytest.raises(_lib.GsplatError, match="shape"):
        gather_foreground(D(m), D(q[:5].clone()), dsplit)
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        gather_foreground(D(torch.rand(3, 7).t()), D(q), dsplit)


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validator_is_sanitizer_clean(tmp_path):
    """gs_scene_loss_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "scene_loss_host_sanitize.c", ["gs_scene_loss_host.cpp", "gs_host.cpp"],
                       "scene loss host sanitize ok")


# ------------------------------------------------------------ the callable and the driver

N_CAMS, HH, WW, P, K = 3, 6, 8, 40, 4
LRS = {"means3D": 1e-3, "rgb_colors": 2e-3, "unnorm_rotations": 1e-3, "logit_opacities": 1e-2, "log_scales": 1e-3}


def _params():
    gen = torch.Generator().manual_seed(5)
    seg = torch.zeros(P, 3)
    seg[:, 0] = (torch.rand(P, generator=gen) < 0.45).float()
    return {"means3D": torch.randn(P, 3, generator=gen), "rgb_colors": torch.rand(P, 3, generator=gen),
            "unnorm_rotations": torch.randn(P, 4, generator=gen), "logit_opacities": torch.randn(P, 1, generator=gen),
            "log_scales": torch.randn(P, 3, generator=gen) * 0.1, "seg_colors": seg}


def _variables(base, graph=True):
    """What initialize_post_first_timestep / initialize_per_timestep leave behind, a little off the
    current state so that every term is non-zero."""
    gen = torch.Generator().manual_seed(9)
    fg = base["seg_colors"][:, 0] > 0.5
    n_fg = int(fg.sum())
    rot = torch.nn.functional.normalize(base["unnorm_rotations"])
    v = {"init_bg_pts": base["means3D"][~fg] + 0.05 * torch.randn(P - n_fg, 3, generator=gen),
         "init_bg_rot": torch.nn.functional.normalize(rot[~fg] + 0.05 * torch.randn(P - n_fg, 4, generator=gen)),
         "prev_col": base["rgb_colors"] + 0.05 * torch.randn(P, 3, generator=gen)}
    if graph:
        v["neighbor_indices"] = torch.randint(0, n_fg, (n_fg, K), generator=gen)
        v["neighbor_weight"] = torch.rand(n_fg, K, generator=gen)
    return v


def _neighbor_stub(fg_pts, fg_rot, variables):
    """A differentiable stand-in for neighbor_losses with its signature (the HIP one needs a device)."""
    nbr, w = variables["neighbor_indices"], variables["neighbor_weight"]
    off = fg_pts[nbr] - fg_pts[:, None]
    rigid = (w * (off ** 2).sum(-1)).mean()
    rot = (w * ((fg_rot[nbr] - fg_rot[:, None]) ** 2).sum(-1)).mean()
    iso = (w * torch.sqrt((off ** 2).sum(-1) + 1e-20)).mean()
    return rigid, rot, iso


@pytest.fixture
def torch_path(monkeypatch):
    """reference_extra_loss with its three HIP calls replaced by torch restatements; counts the calls."""
    calls = {"gather": 0, "neighbor": 0, "reg": 0}

    def gather(means, rot, split):
        calls["gather"] += 1
        return means[split.is_fg], rot[split.is_fg]

    def neighbor(fg_pts, fg_rot, variables):
        calls["neighbor"] += 1
        return _neighbor_stub(fg_pts, fg_rot, variables)

    def reg(means, rot, col, variables, split, **kw):
        calls["reg"] += 1
        return regularizer_losses_torch(means, rot, col, variables, split, **kw)

    monkeypatch.setattr(scene_loss, "gather_foreground", gather)
    monkeypatch.setattr(scene_loss, "neighbor_losses", neighbor)
    monkeypatch.setattr(scene_loss, "regularizer_losses", reg)
    return calls


def _by_hand(params, variables, rv, weights):
    fg = params["seg_colors"][:, 0] > 0.5
    terms = dict(zip(("rigid", "rot", "iso"), _neighbor_stub(rv["means3D"][fg], rv["rotations"][fg], variables)))
    terms.update(zip(("floor", "bg", "soft_col_cons"),
                     regularizer_losses_torch(rv["means3D"], rv["rotations"], params["rgb_colors"], variables, fg)))
    return sum(weights[k] * terms[k] for k in weights), terms


def test_reference_extra_loss_none_logic_and_weights(torch_path):
    base = _params()
    rv = params2rendervar(base)
    fn = reference_extra_loss()
    assert fn(base, _variables(base), rv, 0) is None                      # the initial timestep
    assert fn(base, _variables(base, graph=False), rv, 3) is None         # before the neighbour graph exists
    assert torch_path == {"gather": 0, "neighbor": 0, "reg": 0}
    variables = _variables(base)
    got = fn(base, variables, rv, 1)
    assert scene_loss.WEIGHTS == {"rigid": 0.4, "rot": 0.4, "iso": 0.2, "floor": 0.2, "bg": 2.0, "soft_col_cons": 0.01}
    want, terms = _by_hand(base, variables, rv, scene_loss.WEIGHTS)
    assert all(v.item() > 0 for v in terms.values())
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
    # the split and its mask are cached in `variables`: the second call finds both
    split = variables[scene_loss._SPLIT_KEY][2]
    fn(base, variables, rv, 2)
    assert variables[scene_loss._SPLIT_KEY][2] is split and variables[scene_loss._MASK_KEY][0] is base["seg_colors"]
    base["seg_colors"][0, 0] = 1.0 - base["seg_colors"][0, 0]            # an in-place edit of the seg colours
    variables.update(_variables(base))
    fn(base, variables, rv, 2)
    assert variables[scene_loss._SPLIT_KEY][2] is not split
    # weights: replaced key by key, unknown names refused
    base = _params()
    variables = _variables(base)
    w = dict(scene_loss.WEIGHTS, floor=0.0, bg=3.5)
    got = reference_extra_loss({"floor": 0, "bg": 3.5})(base, variables, rv, 1)
    torch.testing.assert_close(got, _by_hand(base, variables, rv, w)[0], rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="unknown loss names"):
        reference_extra_loss({"rigidity": 1.0})
    # without seg colours every row is foreground: the bg mean is over nothing, NaN as in the reference
    bare = {k: v for k, v in _params().items() if k != "seg_colors"}
    v = _variables(_params())
    v.update(init_bg_pts=torch.zeros(0, 3), init_bg_rot=torch.zeros(0, 4), neighbor_indices=torch.randint(0, P, (P, K)),
             neighbor_weight=torch.rand(P, K))
    assert torch.isnan(reference_extra_loss()(bare, v, rv, 1))
    assert v[scene_loss._SPLIT_KEY][2].n_fg == P


def _stub_render():
    """A differentiable stand-in for the rasterizer: every pixel a fixed mix of the Gaussians."""
    gen = torch.Generator().manual_seed(6)
    mix = torch.softmax(3.0 * torch.randn(N_CAMS, HH * WW, P, generator=gen), dim=-1)

    def render(rv, cams):
        col = rv["colors_precomp"] * rv["opacities"]
        return torch.stack([(mix[c] @ col).t().reshape(3, HH, WW) for c in cams]), None
    return render


def _drive(t, steps=2, variables=None, **kw):
    params = {k: torch.nn.Parameter(v.clone()) if k in LRS else v.clone() for k, v in _params().items()}
    opt = torch.optim.Adam([{"params": [params[k]], "name": k, "lr": lr} for k, lr in LRS.items()], lr=0.0, eps=1e-15)
    drv = TimestepDriver(params, {} if variables is None else variables, opt, N_CAMS, render=_stub_render(), **kw)
    tg = torch.rand(N_CAMS, 3, HH, WW, generator=torch.Generator().manual_seed(7))
    losses = [drv.step(tg, t, i) for i in range(steps)]
    return losses, {k: v.detach().clone() for k, v in drv.params.items()}, tg


def test_driver_without_the_callable_is_unchanged():
    """extra_loss=None: two steps are bit-identical to the run without the argument (the driver is
    not modified; importing scene_loss changes nothing about it)."""
    base = _drive(1)
    got = _drive(1, extra_loss=None, variables=_variables(_params()))
    assert got[0] == base[0]
    for k in base[1]:
        assert torch.equal(got[1][k], base[1][k]), k


def test_driver_adds_the_block_once(torch_path):
    variables = _variables(_params())
    losses, after, tg = _drive(1, steps=1, variables=variables, extra_loss=reference_extra_loss())
    assert torch_path == {"gather": 1, "neighbor": 1, "reg": 1}
    # the same step by hand
    params = {k: torch.nn.Parameter(v.clone()) if k in LRS else v.clone() for k, v in _params().items()}
    rv = params2rendervar(params)
    ims, _ = _stub_render()(rv, list(range(N_CAMS)))
    image_term = l1_image_loss(ims, tg) / N_CAMS
    block, _ = _by_hand(params, _variables(_params()), rv, scene_loss.WEIGHTS)
    want = image_term + block
    assert block.item() > 0 and losses[0] == pytest.approx(want.item(), rel=1e-6)
    opt = torch.optim.Adam([{"params": [params[k]], "name": k, "lr": lr} for k, lr in LRS.items()], lr=0.0, eps=1e-15)
    want.backward()
    opt.step()
    for k in LRS:
        torch.testing.assert_close(after[k], params[k].detach(), rtol=1e-6, atol=1e-9)
    without, _, _ = _drive(1, steps=1)
    assert without[0] == pytest.approx(image_term.item(), rel=1e-6) and without[0] != losses[0]
