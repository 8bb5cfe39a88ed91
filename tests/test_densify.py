"""CPU tests of densification (no GPU needed):
  * densify_torch reproduces every case of the fixture tests/golden/densify.npz,
    recorded from the reference's external.py by tests/golden/make_golden_densify.py:
    length and row order exactly, copied rows, moments and step counts bit for bit, the
    split means and log-scales to rtol 1e-6 / atol 1e-7 (a few fp32 ulps of a
    three-operation chain);
  * the schedule over i in {0, 499, 500, 550, 2900, 3000, 5000, 5100, 6000};
  * semantic_feature (width 32) and a group-less seg_colors are compacted with means3D;
  * the library exports every symbol include/gs_densify.h declares, each with a ctypes
    prototype; the ctypes mirrors have the library's sizes and the header's fields; ABI 13;
  * the host validators refuse every bad argument block with a message, and the entry
    points run them before touching a device;
  * the wrapper refuses what the kernels cannot take (no CPU fallback);
  * the validators run clean under AddressSanitizer + UndefinedBehaviorSanitizer in a
    stand-alone program (tools/densify_host_sanitize.c).
"""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dynamic3dgaussians_amd import _lib, densify, densify_torch
from tests import _densify_cases as C
from tests._harness import run_host_sanitizer

D = importlib.import_module("dynamic3dgaussians_amd.densify")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gs_densify.h")


@pytest.fixture(scope="module")
def gold():
    return np.load(C.GOLD)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(C.GOLD) < 512 * 1024
    for name in C.CASES:
        for k in C.KEYS + C.CAM_KEYS:
            for suffix in ("", ".exp_avg", ".exp_avg_sq", ".step"):
                assert f"{name}.in.{k}{suffix}" in gold and f"{name}.out.{k}{suffix}" in gold, (name, k, suffix)
            assert gold[f"{name}.in.{k}"].dtype == np.float32
        for k in C.STATS:
            assert f"{name}.in.{k}" in gold and f"{name}.out.{k}" in gold
    assert gold["i500.in.means3D"].shape[0] == 300
    # the structural cases change the length, clone and split; the others do not
    for name in ("i500", "i3000", "i5000"):
        assert gold[f"{name}.out.means3D"].shape[0] != gold[f"{name}.in.means3D"].shape[0]
        assert gold[f"{name}.z"].shape[0] > 0 and gold[f"{name}.z"].shape[1] == 3
    for name in ("i550", "i600"):
        assert gold[f"{name}.out.means3D"].shape[0] == gold[f"{name}.in.means3D"].shape[0]
        assert gold[f"{name}.z"].shape[0] == 0
    assert (gold["i3000.out.logit_opacities"] == gold["i3000.out.logit_opacities"][0]).all()  # the reset


@pytest.mark.parametrize("name", C.CASES)
def test_fixture_keeps_its_margins(gold, name):
    parts, i, _z = C.fixture_parts(gold, name)
    seen = parts["seen"]
    acc, den = parts["stats"]["means2D_gradient_accum"].clone(), parts["stats"]["denom"].clone()
    acc[seen] += torch.norm(parts["means2D_grad"][seen, :2], dim=-1)
    den[seen] += 1
    C.assert_margins(parts["tensors"]["log_scales"], parts["tensors"]["logit_opacities"], acc, den,
                     parts["scene_radius"], i, exact_rows=0 if name == "i600" else 1)


@pytest.mark.parametrize("name", C.CASES)
def test_torch_restatement_reproduces_the_reference(gold, name):
    parts, i, z = C.fixture_parts(gold, name)
    params, variables, opt = C.build(**parts)
    before = dict(params)
    params, variables = densify_torch(params, variables, opt, i, noise=z if z.numel() else None)
    got = C.snapshot(params, variables, opt)
    want = {k[len(name) + 5:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(f"{name}.out.")}
    assert set(want) <= set(got)
    n_in = gold[f"{name}.in.means3D"].shape[0]
    structural = name != "i550"  # i600 runs the pass too: nothing qualifies, new Parameters all the same
    splits = gold[f"{name}.z"].shape[0] > 0
    for k, w in want.items():
        g = got[k]
        assert tuple(g.shape) == tuple(w.shape), (k, g.shape, w.shape)  # the output length
        if k in C.TRANSFORMED and splits:
            # a row that exists in the input is a copy (a kept original or a clone): bit for bit;
            # the others are split copies and carry the formulas
            rows_in = torch.from_numpy(gold[f"{name}.in.{k}"])
            is_copy = (w[:, None, :] == rows_in[None]).all(-1).any(-1)
            assert 0 < int((~is_copy).sum()) <= gold[f"{name}.z"].shape[0]
            assert torch.equal(g[is_copy], w[is_copy]), k
            torch.testing.assert_close(g, w, rtol=1e-6, atol=1e-7)
        else:
            assert torch.equal(g, w), k  # copied rows, moments, step counts, statistics: bit for bit
    for k in C.KEYS:
        replaced = params[k] is not before[k]
        assert replaced == (structural or (name == "i3000" and k == "logit_opacities")), k
        if replaced:
            assert isinstance(params[k], torch.nn.Parameter) and params[k].grad is None
            assert [g for g in opt.param_groups if g["name"] == k][0]["params"][0] is params[k]
    for k in C.CAM_KEYS:
        assert params[k] is before[k]
    assert n_in == before["means3D"].shape[0]


def _tiny(seed=5, P=40, **kw):
    parts = C.random_parts(P, seed, **kw)
    C.parts_margins(parts, 500)
    return parts


@pytest.mark.parametrize("i", [0, 499, 500, 550, 2900, 3000, 5000, 5100, 6000])
def test_schedule(i):
    sch = D.schedule(i)
    assert sch["active"] == (i <= 5000)
    assert sch["structure"] == (i in (500, 2900, 3000, 5000))
    assert sch["reset"] == (i == 3000)
    assert sch["remove_threshold"] == (0.25 if i == 5000 else 0.005)
    assert sch["big_points"] == (i >= 3000)
    # and what densify_torch does with it
    parts = _tiny()
    P = parts["tensors"]["means3D"].shape[0]
    parts["seen"] = torch.ones(P, dtype=torch.bool)
    parts["means2D_grad"] = torch.zeros(P, 3)
    params, variables, opt = C.build(**parts)
    before, denom0 = dict(params), variables["denom"].clone()
    params, variables = densify_torch(params, variables, opt, i, generator=torch.Generator().manual_seed(0))
    if i > 5000:
        assert all(params[k] is before[k] for k in before) and torch.equal(variables["denom"], denom0)
        return
    if sch["structure"]:
        assert all(params[k] is not before[k] for k in C.KEYS)
        assert params["means3D"].shape[0] != P  # this case clones, splits and prunes
        assert not variables["denom"].any() and variables["denom"].shape[0] == params["means3D"].shape[0]
    else:
        assert all(params[k] is before[k] for k in C.KEYS)
        assert torch.equal(variables["denom"], denom0 + 1)  # accumulate only
    if sch["reset"]:
        assert bool((torch.sigmoid(params["logit_opacities"]) - 0.01).abs().max() < 1e-6)
        st = opt.state[params["logit_opacities"]]
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) > 0


def test_accumulate_flag_and_generator():
    parts = _tiny()
    P = parts["tensors"]["means3D"].shape[0]
    parts["seen"] = torch.ones(P, dtype=torch.bool)
    parts["means2D_grad"] = torch.ones(P, 3)
    params, variables, opt = C.build(**parts)
    denom0 = variables["denom"].clone()
    densify_torch(params, variables, opt, 550, accumulate=False)
    assert torch.equal(variables["denom"], denom0)
    outs = []
    for _ in range(2):
        params, variables, opt = C.build(**parts)
        params, variables = densify_torch(params, variables, opt, 500, accumulate=False,
                                          generator=torch.Generator().manual_seed(7))
        outs.append(params["means3D"].detach().clone())
    assert torch.equal(outs[0], outs[1])


def test_semantic_feature_and_groupless_tensors_follow_means3D():
    """Width-32 semantic_feature keeps its optimizer group and state (the reference's
    remove_points drops it: a documented departure); a seg_colors without a group is
    compacted as a plain tensor.  Row r of every output comes from the same source row."""
    parts = _tiny(seed=9, P=60, extra={"semantic_feature": 32})
    P = 60
    tag = torch.arange(P, dtype=torch.float32)
    parts["tensors"]["semantic_feature"][:, 0] = tag
    parts["tensors"]["seg_colors"][:, 0] = tag
    parts["tensors"]["rgb_colors"][:, 0] = tag
    parts["moments"].pop("seg_colors")
    params, variables, opt = C.build(**parts, no_group=("seg_colors",))
    params, variables = densify_torch(params, variables, opt, 500, accumulate=False,
                                      generator=torch.Generator().manual_seed(1))
    n = params["means3D"].shape[0]
    assert n != P
    for k in ("semantic_feature", "seg_colors", "rgb_colors"):
        assert params[k].shape[0] == n
        assert torch.equal(params[k][:, 0].detach(), params["rgb_colors"][:, 0].detach()), k
    assert isinstance(params["semantic_feature"], torch.nn.Parameter)
    assert not isinstance(params["seg_colors"], torch.nn.Parameter) and not params["seg_colors"].requires_grad
    sf = opt.state[params["semantic_feature"]]
    assert sf["exp_avg"].shape == (n, 32) and float(sf["step"]) == parts["steps"]["semantic_feature"]
    # originals keep their moments, every new row starts from zero
    src = params["rgb_colors"][:, 0].detach().long()
    first_new = int((src[1:] < src[:-1]).nonzero()[0]) + 1 if bool((src[1:] < src[:-1]).any()) else n
    assert torch.equal(sf["exp_avg"][:first_new], parts["moments"]["semantic_feature"][0][src[:first_new]])
    assert not sf["exp_avg"][first_new:].any() and not sf["exp_avg_sq"][first_new:].any()


# ---- the C ABI ----

def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_library_exports_every_symbol_of_gs_densify_h():
    L = _lib.load()
    names = sorted(set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", _header_text())))
    assert {"gs_densify_plan", "gs_densify_apply", "gs_densify_workspace_bytes", "gs_densify_plan_validate",
            "gs_densify_apply_validate", "gs_densify_plan_struct_bytes"} <= set(names)
    for n in names:
        assert hasattr(L, n), n
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (gs_[a-z_0-9]+)", out))
    assert L.gs_version() == _lib.ABI_VERSION == 13  # a new header, no existing struct changed


@pytest.mark.parametrize("struct,mirror,size_fn", [
    ("gs_densify_plan_args", "GsDensifyPlanArgs", "gs_densify_plan_struct_bytes"),
    ("gs_densify_tensor", "GsDensifyTensor", "gs_densify_tensor_struct_bytes"),
    ("gs_densify_apply_args", "GsDensifyApplyArgs", "gs_densify_apply_struct_bytes")])
def test_ctypes_mirrors_have_the_library_sizes_and_the_header_fields(struct, mirror, size_fn):
    L = _lib.load()
    cls = getattr(_lib, mirror)
    assert ctypes.sizeof(cls) == getattr(L, size_fn)()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header_text(), flags=re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        for part in decl.split(","):
            names.append(re.findall(r"[A-Za-z_]\w*", re.sub(r"\[.*?\]", "", part))[-1])
    assert [f for f, _ in cls._fields_] == names
    assert _lib.GS_DENSIFY_MAX_TENSORS == 16 and ctypes.sizeof(_lib.GsDensifyApplyArgs().t) == 16 * ctypes.sizeof(
        _lib.GsDensifyTensor)


def test_workspace_geometry():
    L = _lib.load()
    B = L.gs_densify_scan_block()
    assert B > 0 and L.gs_densify_scan_tile() > 0
    for P in (1, 63, B, B + 1, 3 * B + 17, 300_000):
        ws = L.gs_densify_workspace_bytes(P)
        blocks = (P + B - 1) // B
        assert 17 * P + 32 + 16 * blocks <= ws <= 17 * P + 32 + 16 * blocks + 2048
        assert L.gs_densify_counts_offset(P) + 32 <= L.gs_densify_flags_offset(P)
        assert L.gs_densify_flags_offset(P) + P <= L.gs_densify_ranks_offset(P)
        assert L.gs_densify_ranks_offset(P) % 16 == 0 and L.gs_densify_ranks_offset(P) + 16 * P <= ws
    assert L.gs_densify_workspace_bytes(0) == 0 and L.gs_densify_workspace_bytes(-3) == 0
    counts = (ctypes.c_int64 * 4)(5, 3, 9, 4)
    assert L.gs_densify_new_count(counts, 2) == 5 + 3 + 8


def _good_blocks(keep):
    """Valid plan and apply blocks over host arrays (the validators dereference nothing)."""
    L = _lib.load()
    P, counts = 3000, (2000, 1000, 600, 500)
    P_new = counts[0] + counts[1] + 2 * counts[3]
    ws_bytes = L.gs_densify_workspace_bytes(P)
    bufs = {"src": np.zeros(P * 4, np.float32), "dst": np.zeros(P_new * 4, np.float32),
            "mom": np.zeros(P * 4, np.float32), "dmom": np.zeros(P_new * 4, np.float32),
            "noise": np.zeros(2 * P * 3, np.float32), "stat": np.zeros(P_new, np.float32),
            "ws": np.zeros(ws_bytes // 4 + 128, np.float32)}
    keep.append(bufs)
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["ws"] = (p["ws"] + 255) // 256 * 256
    plan = _lib.GsDensifyPlanArgs(P=P, grad_accum=p["src"], denom=p["src"], log_scales=p["src"],
                                  logit_opacities=p["src"], grad_thresh=0.0002, clone_max_scale=0.02,
                                  prune_min_opacity=0.005, prune_max_scale=0.0, n_split=2, workspace=p["ws"],
                                  workspace_bytes=ws_bytes)
    apply = _lib.GsDensifyApplyArgs(P=P, workspace=p["ws"], workspace_bytes=ws_bytes, n_split=2, n_tensors=5,
                                    noise=p["noise"], opacity_reset=-4.595)
    for j in range(4):
        apply.counts[j] = counts[j]
    for j in range(3):
        apply.stats[j] = p["stat"]
    for t, (role, width) in enumerate([("means", 3), ("log_scales", 3), ("rotations", 4), ("logit_opacities", 1),
                                       ("plain", 32)]):
        x = apply.t[t]
        x.src, x.dst, x.src_exp_avg, x.src_exp_avg_sq = p["src"], p["dst"], p["mom"], p["mom"]
        x.dst_exp_avg, x.dst_exp_avg_sq = p["dmom"], p["dmom"]
        x.width, x.role = width, _lib.GS_DENSIFY_ROLES[role]
    return plan, apply, p


def test_validators_reject_bad_arguments_without_gpu():
    L = _lib.load()
    keep = []
    plan, apply, p = _good_blocks(keep)
    assert L.gs_densify_plan_validate(ctypes.byref(plan)) == 0
    assert L.gs_densify_apply_validate(ctypes.byref(apply)) == 0
    assert L.gs_densify_plan_validate(None) < 0 and b"null argument" in L.gs_last_error()
    assert L.gs_densify_apply_validate(None) < 0 and b"null argument" in L.gs_last_error()
    inf, nan = float("inf"), float("nan")
    for field, value, msg in [("P", -1, b"P must be"), ("n_split", 3, b"n_split"), ("n_split", 1, b"n_split"),
                              ("grad_thresh", nan, b"finite"), ("clone_max_scale", inf, b"finite"),
                              ("prune_min_opacity", -inf, b"finite"), ("prune_max_scale", nan, b"finite"),
                              ("grad_accum", None, b"required"), ("logit_opacities", None, b"required"),
                              ("log_scales", p["src"] + 2, b"4-byte aligned"), ("denom", p["src"] + 1, b"4-byte"),
                              ("workspace", None, b"workspace is required"), ("workspace_bytes", 64, b"needed"),
                              ("workspace", p["ws"] + 4, b"16-byte aligned")]:
        bad, _, _ = _good_blocks(keep)
        setattr(bad, field, value)
        assert L.gs_densify_plan_validate(ctypes.byref(bad)) < 0, (field, value)
        assert msg in L.gs_last_error(), (field, L.gs_last_error())

    def tensor(t, **kw):
        def edit(a):
            for k, v in kw.items():
                setattr(a.t[t], k, v)
        return edit

    def top(**kw):
        def edit(a):
            for k, v in kw.items():
                setattr(a, k, v)
        return edit

    def count(j, v):
        def edit(a):
            a.counts[j] = v
        return edit

    def stat(j, v):
        def edit(a):
            a.stats[j] = v
        return edit

    means, plain = _lib.GS_DENSIFY_ROLES["means"], _lib.GS_DENSIFY_ROLES["plain"]
    for edit, msg in [(top(P=-2), b"P must be"), (top(n_split=4), b"n_split"), (top(n_tensors=17), b"n_tensors"),
                      (top(n_tensors=-1), b"n_tensors"), (count(3, 700), b"counts"), (count(0, -1), b"counts"),
                      (count(0, 3000), b"counts"), (tensor(2, width=0), b"width"), (tensor(4, width=-3), b"width"),
                      (tensor(1, width=4), b"has width"), (tensor(4, role=9), b"unknown role"),
                      (tensor(4, role=means, width=3), b"used twice"), (tensor(3, role=plain), b"is missing"),
                      (top(n_tensors=0), b"is missing"), (tensor(0, src=None), b"src is required"),
                      (tensor(0, dst=None), b"dst is required"), (tensor(4, dst=p["dst"] + 1), b"4-byte aligned"),
                      (tensor(4, src=p["src"] + 2), b"4-byte aligned"),
                      (tensor(4, src_exp_avg=p["mom"] + 3), b"4-byte aligned"),
                      (tensor(4, dst_exp_avg_sq=None), b"come together"), (top(noise=None), b"noise is required"),
                      (top(noise=p["noise"] + 2), b"4-byte aligned"), (stat(1, p["stat"] + 1), b"4-byte aligned"),
                      (top(reset_opacity=1, opacity_reset=nan), b"finite"),
                      (top(workspace=None), b"workspace is required"), (top(workspace_bytes=100), b"needed"),
                      (top(workspace=p["ws"] + 8), b"16-byte aligned")]:
        _, bad, _ = _good_blocks(keep)
        edit(bad)
        assert L.gs_densify_apply_validate(ctypes.byref(bad)) < 0, msg
        assert msg in L.gs_last_error(), (msg, L.gs_last_error())
    # a tensor without optimizer state, or whose state does not exist yet
    _, lazy, _ = _good_blocks(keep)
    lazy.t[4].src_exp_avg = lazy.t[4].src_exp_avg_sq = None
    assert L.gs_densify_apply_validate(ctypes.byref(lazy)) == 0
    lazy.t[4].dst_exp_avg = lazy.t[4].dst_exp_avg_sq = None
    assert L.gs_densify_apply_validate(ctypes.byref(lazy)) == 0
    # the entry points run the validators before anything touches a device
    bad, bad_apply, _ = _good_blocks(keep)
    bad.n_split = 5
    assert L.gs_densify_plan(ctypes.byref(bad), None) < 0 and b"n_split" in L.gs_last_error()
    bad_apply.n_tensors = 40
    assert L.gs_densify_apply(ctypes.byref(bad_apply), None) < 0 and b"n_tensors" in L.gs_last_error()
    # nothing to do: no launch, no device
    none = _lib.GsDensifyPlanArgs(P=0, n_split=2)
    assert L.gs_densify_plan(ctypes.byref(none), None) == 0
    _, empty, _ = _good_blocks(keep)
    for j in range(4):
        empty.counts[j] = 0
    assert L.gs_densify_apply(ctypes.byref(empty), None) == 0  # P_new = 0


class _DeviceClaim(torch.Tensor):
    """A host tensor that reports is_cuda, so the wrapper's dtype / layout / shape rules (all
    checked before any device work) can be exercised where there is no GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    @property
    def is_cuda(self):
        return True


def test_wrapper_rejects_what_the_kernels_cannot_take():
    parts = _tiny()
    params, variables, opt = C.build(**parts)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        densify(params, variables, opt, 500, accumulate=False)
    with pytest.raises(_lib.GsplatError, match="device tensors"):
        D.plan(variables["means2D_gradient_accum"], variables["denom"], params["log_scales"].detach(),
               params["logit_opacities"].detach(), grad_thresh=2e-4, clone_max_scale=0.02, prune_min_opacity=0.005)
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(_lib.GsplatError, match="float32"):
            D._need(_DeviceClaim(torch.rand(8, 3).to(dtype)), "means3D")
    with pytest.raises(_lib.GsplatError, match="contiguous"):
        D._need(_DeviceClaim(torch.rand(3, 8).t()), "means3D")
    with pytest.raises(_lib.GsplatError, match="rows"):
        D._need(_DeviceClaim(torch.rand(7, 3)), "rgb_colors", 8)
    with pytest.raises(_lib.GsplatError, match="must be a tensor"):
        D._need([1.0], "means3D")

    def claimed(**replace):
        params, variables, opt = C.build(**parts)
        params = {k: _DeviceClaim(v.detach()) for k, v in params.items()}
        variables = {k: _DeviceClaim(v) if isinstance(v, torch.Tensor) else v for k, v in variables.items()}
        for k, v in replace.items():
            (variables if k in C.STATS else params)[k] = _DeviceClaim(v)
        return params, variables, None

    P = parts["tensors"]["means3D"].shape[0]
    for replace, msg in [({"rgb_colors": torch.rand(P, 3).double()}, "float32"),
                         ({"means3D": torch.rand(3, P).t()}, "contiguous"),
                         ({"seg_colors": torch.rand(P + 1, 3)}, "rows"),
                         ({"denom": torch.rand(P).half()}, "float32"),
                         ({"means2D_gradient_accum": torch.rand(P - 1)}, "rows")]:
        with pytest.raises(_lib.GsplatError, match=msg):
            densify(*claimed(**replace), 500, accumulate=False)
    many = claimed()
    for n in range(12):
        many[0][f"extra{n}"] = _DeviceClaim(torch.rand(P, 2))
    with pytest.raises(_lib.GsplatError, match="at most 16"):
        densify(*many, 500, accumulate=False)
    missing = claimed()
    del missing[0]["unnorm_rotations"]
    with pytest.raises(_lib.GsplatError, match="unnorm_rotations"):
        densify(*missing, 500, accumulate=False)
    # beyond the schedule nothing is looked at
    out = densify(params, variables, opt, 5001)
    assert out[0] is params and out[1] is variables


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="gcc / g++ not available")
def test_validators_are_sanitizer_clean(tmp_path):
    """gs_densify_host.cpp (with gs_host.cpp's error state) under ASan + UBSan in a plain CPU
    executable with its own main: nothing preloaded, nothing loaded into Python."""
    run_host_sanitizer(tmp_path, "densify_host_sanitize.c", ["gs_densify_host.cpp", "gs_host.cpp"],
                       "densify host sanitize ok")
