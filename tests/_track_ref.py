"""The reference for the contributor maps (include/gs_track.h): a float64 numpy
replay of the forward's blend chain (CR/forward.cu:350-380) over the CPU
oracle's records -- OracleState.means2D, conic_opacity, ranges and point_list
from tests._harness.oracle_forward.  Per tile the [list entry, pixel]
arithmetic is vectorised; the chain's only sequential quantity, the
transmittance, is a cumulative product: before the walk ends every candidate
entry blends, so T after entry i is the product of (1 - alpha) over the
candidates up to i, and the walk ends at the first candidate whose product
falls under 1e-4 (that entry is not blended).

The constants are the forward's fp32 constants (1/255, 0.99, 1e-4) read as
doubles; everything else is fp64 on the oracle's fp32 records."""
from __future__ import annotations

import functools

import numpy as np

from tests import _harness as H

ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))
ALPHA_MAX = float(np.float32(0.99))
T_MIN = float(np.float32(0.0001))
TILE = 16


def replay_tiles(st, W, H_):
    """Yields, per non-empty tile, (ids [n] in list order, w [n, h, w] float64 -- 0 where the
    entry does not blend at the pixel --, y0, x0)."""
    m2 = np.asarray(st.means2D, np.float64)
    co = np.asarray(st.conic_opacity, np.float64)
    ranges = np.asarray(st.ranges, np.int64).reshape(-1, 2)
    plist = np.asarray(st.point_list, np.int64)
    gx = (W + TILE - 1) // TILE
    for t in range(ranges.shape[0]):
        lo, hi = ranges[t]
        if hi <= lo:
            continue
        ids = plist[lo:hi]
        x0, y0 = (t % gx) * TILE, (t // gx) * TILE
        xs = np.arange(x0, min(x0 + TILE, W), dtype=np.float64)
        ys = np.arange(y0, min(y0 + TILE, H_), dtype=np.float64)
        px, py = np.meshgrid(xs, ys)
        dx = m2[ids, 0, None, None] - px[None]
        dy = m2[ids, 1, None, None] - py[None]
        a, b, c, op = (co[ids, k, None, None] for k in range(4))
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        alpha = np.minimum(ALPHA_MAX, op * np.exp(np.minimum(power, 0.0)))
        cand = (power <= 0.0) & (alpha >= ALPHA_MIN)
        t_after = np.cumprod(np.where(cand, 1.0 - alpha, 1.0), axis=0)  # T after entry i, were it blended
        t_before = np.concatenate([np.ones_like(t_after[:1]), t_after[:-1]], axis=0)
        ended = np.cumsum(cand & (t_after < T_MIN), axis=0) > 0  # from the first saturating candidate on
        w = np.where(cand & ~ended, alpha * t_before, 0.0)
        yield ids, w, y0, x0


def replay(st, W, H_, K):
    """The replay's maps: (top_id int64 [K, H, W], top_w float64 [K + 1, H, W] -- one rank more
    than the ids, for the gap between ranks K - 1 and K --, alpha float64 [H, W] = the sum of all
    weights, count int64 [H, W] = blended entries).  Between equal weights the earlier entry."""
    top_id = np.full((K, H_, W), -1, np.int64)
    top_w = np.zeros((K + 1, H_, W), np.float64)
    alpha = np.zeros((H_, W), np.float64)
    count = np.zeros((H_, W), np.int64)
    for ids, w, y0, x0 in replay_tiles(st, W, H_):
        n, h, ww = w.shape
        order = np.argsort(-w, axis=0, kind="stable")[:K + 1]  # largest first, list order between equals
        ws = np.take_along_axis(w, order, axis=0)
        k1 = min(K + 1, n)
        top_w[:k1, y0:y0 + h, x0:x0 + ww] = ws[:k1]
        k0 = min(K, n)
        top_id[:k0, y0:y0 + h, x0:x0 + ww] = np.where(ws[:k0] > 0.0, ids[order[:k0]], -1)
        alpha[y0:y0 + h, x0:x0 + ww] = w.sum(axis=0)
        count[y0:y0 + h, x0:x0 + ww] = (w > 0.0).sum(axis=0)
    return top_id, top_w, alpha, count


def robust(top_w, k, rel=1e-3):
    """Pixels whose rank k is decided by more than rounding: the replay's weights at ranks k and
    k + 1 differ by more than `rel` of the larger.  A pixel without a rank-k entry (both 0) is
    robust: nothing can rank there."""
    a, b = top_w[k], top_w[k + 1]
    return (a - b > rel * a) | (a == 0.0)


# scenes of the tracking tests (tests._harness.scene keywords), and their shared references
SCENES = {
    "p2000": dict(P=2000, W=128, H=96),
    "edges": dict(P=2000, seed=3, W=100, H=70),
    "long": dict(P=800, scale_mult=6.0, W=128, H=96),
}


@functools.lru_cache(maxsize=None)
def scene(name, cam_index=0):
    return H.scene(cam_index=cam_index, **SCENES[name])


@functools.lru_cache(maxsize=None)
def oracle(name, cam_index=0, compat="fixed"):
    return H.oracle_forward(scene(name, cam_index), compat=compat)


@functools.lru_cache(maxsize=None)
def reference(name, cam_index=0, K=4):
    """(top_id, top_w, alpha, count) of the replay over the oracle's records; computed once per
    scene and camera and shared (read-only) by the tests."""
    kw = SCENES[name]
    out = replay(oracle(name, cam_index)[6], kw["W"], kw["H"], K)
    for a in out:
        a.setflags(write=False)
    return out
