"""Seeded inputs of the depth-geometry tests and of tests/golden/make_golden_depth_geometry.py
(CPU torch; every value is drawn in fp64 and rounded to fp32 once, so fp32 and fp64 runs see
the same numbers).

Cameras are pinholes without skew (ideaII.pixel_to_camera_coordinates reads fx, fy, cx, cy
only) with fx != fy and off-centre principal points, under small rotations.

robust_cloud builds a point cloud backwards from the pixels so that no decision of the
z-buffer hangs on rounding: an integer target pixel in [-3, W + 3) x [-3, H + 3), a jitter of
at most 0.4 pixel (the nearest rounding tie is 0.1 pixel away; fp32 moves u by ~1e-5), a depth
in [0.5, 4.5] negated for every 17th point, unprojected in fp64 and cast to fp32.
"""
import math

import torch

ZBUF_CASES = {"zbuf_5x7": (5, 7, 1000, 41), "zbuf_37x53": (37, 53, 4097, 42)}  # H, W, P, seed
FLOW_CASES = {"flow_5x7": (5, 7, 51), "flow_37x53": (37, 53, 52)}  # H, W, seed


def f32(x):
    """Rounded to fp32 once, kept as fp64."""
    return x.float().double()


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    X = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Y = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Z = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return Z @ Y @ X


def rigid(R, t):
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = R
    m[:3, 3] = torch.as_tensor(t, dtype=torch.float64)
    return m


def pinhole(H, W, k):
    """The k-th intrinsics of an H x W image: fx != fy, principal point off the centre."""
    fx, fy = W * (0.9 + 0.15 * k), W * (1.1 - 0.1 * k)
    return f32(torch.tensor([[fx, 0, W / 2 - 0.7 + 0.9 * k], [0, fy, H / 2 + 0.4 - 0.6 * k], [0, 0, 1]],
                            dtype=torch.float64))


def zbuf_cameras(H, W):
    """(w2c [2, 4, 4], K [2, 3, 3]) fp64 holding fp32 values: two differently rotated cameras."""
    w2c = torch.stack([rigid(rotation(0.11, -0.23, 0.05), (0.2, -0.1, 0.3)),
                       rigid(rotation(-0.17, 0.31, -0.09), (-0.3, 0.15, 0.1))])
    return f32(w2c), torch.stack([pinhole(H, W, 0), pinhole(H, W, 1)])


def robust_cloud(w2c, K, H, W, P, seed):
    """[B, P, 3] fp32: one decision-robust cloud per camera (module docstring)."""
    gen = torch.Generator().manual_seed(seed)
    clouds = []
    for b in range(w2c.shape[0]):
        px = torch.randint(-3, W + 3, (P,), generator=gen).double()
        py = torch.randint(-3, H + 3, (P,), generator=gen).double()
        jit = (torch.rand(P, 2, generator=gen, dtype=torch.float64) - 0.5) * 0.8
        z = 0.5 + 4.0 * torch.rand(P, generator=gen, dtype=torch.float64)
        z[::17] = -z[::17]
        pix = torch.stack([px + jit[:, 0], py + jit[:, 1], torch.ones(P, dtype=torch.float64)], dim=-1)
        cam = z[:, None] * (pix @ torch.linalg.inv(K[b]).T)
        c2w = torch.linalg.inv(w2c[b])
        clouds.append((cam @ c2w[:3, :3].T + c2w[:3, 3]).float())
    return torch.stack(clouds).contiguous()


def zbuf_case(name):
    """points [2, P, 3] fp32, w2c, K (fp64 of fp32 values), gt [2, H, W] fp32, exclude [2, H, W] uint8."""
    H, W, P, seed = ZBUF_CASES[name]
    w2c, K = zbuf_cameras(H, W)
    pts = robust_cloud(w2c, K, H, W, P, seed)
    gen = torch.Generator().manual_seed(seed + 100)
    gt = 0.4 + 4.0 * torch.rand(2, H, W, generator=gen, dtype=torch.float32)
    gt[torch.rand(2, H, W, generator=gen, dtype=torch.float32) < 0.1] = 0.0  # no ground truth there
    exclude = (torch.rand(2, H, W, generator=gen, dtype=torch.float32) < 0.3).to(torch.uint8)
    return pts, w2c, K, gt, exclude


def flow_cameras(away=False):
    """(c2w1, w2c2) fp64 of fp32 values: two small rotations per camera, camera 2 moved 0.6
    forward; away=True turns camera 2 round (every point behind it)."""
    c2w1 = rigid(rotation(0.04, -0.06, 0.0), (0.05, -0.02, 0.0))
    R2 = rotation(-0.05, 0.03 + (math.pi if away else 0.0), 0.0)
    w2c2 = rigid(R2, (0.03, 0.04, -0.6))
    return f32(c2w1), f32(w2c2)


def flow_case(name, away=False):
    """depth1 [H, W] fp32 in [1.4, 3] with two zero pixels, K1, c2w1, K2, w2c2."""
    H, W, seed = FLOW_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    depth = 1.4 + 1.6 * torch.rand(H, W, generator=gen, dtype=torch.float32)
    depth[1, 2] = 0.0
    depth[H - 2, W - 3] = 0.0
    c2w1, w2c2 = flow_cameras(away)
    return depth, pinhole(H, W, 0), c2w1, pinhole(H, W, 1), w2c2


def flows(H, W, n, seed):
    """n smooth flows [n, 2, H, W] fp32 of a few pixels' amplitude, some of it past the border."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float32), torch.linspace(0, 1, W, dtype=torch.float32),
                            indexing="ij")
    f = torch.rand(n, 2, 4, generator=gen, dtype=torch.float32)[..., None, None] * 5.0
    base = 2.5 * torch.sin(f[:, :, 0] * xx + f[:, :, 1]) * torch.cos(f[:, :, 2] * yy + f[:, :, 3])
    return (base + 0.3 * torch.randn(n, 2, H, W, generator=gen, dtype=torch.float32)).float().contiguous()
