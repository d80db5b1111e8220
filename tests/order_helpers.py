"""Shared by the coherent-order tests (test_order_host.py, test_gpu_order.py): the key of rfx.h "Coherent order"
restated in numpy float32, and the rays that probe its edges.

Every step below is one IEEE float32 operation, as the device's are (no contraction), so the restatement gives the
key bit for bit.  np.fmax / np.fmin are fmaxf / fminf: a NaN operand is ignored, so a NaN takes the 0.
"""
from __future__ import annotations

import numpy as np

from reflaxman_amd import _lib

CB, DB = _lib.RFX_ORDER_CELL_BITS, _lib.RFX_ORDER_DIR_BITS
F = np.float32


def scene_box(desc):
    """(lo, scale) of a scene description as rfx_renderer_set_scene computes them: float32, insertion order, planes
    left out; scale 0 (and a non-finite lo given as 0) where the box is empty or flat."""
    lo, hi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    for ob in desc.objects:
        if ob[0] == "sphere":
            c, r = np.asarray(ob[1], F), F(ob[2])
            lo, hi = np.fmin(lo, c - r), np.fmax(hi, c + r)
        elif ob[0] == "triangle":
            for v in ob[1:4]:
                v = np.asarray(v, F)
                lo, hi = np.fmin(lo, v), np.fmax(hi, v)
    ok = (hi > lo) & np.isfinite(lo) & np.isfinite(hi)
    with np.errstate(all="ignore"):
        scale = np.where(ok, F(1 << CB) / (hi - lo), F(0)).astype(F)
    return np.where(np.isfinite(lo), lo, F(0)).astype(F), scale


def _spread(x, step, bits):
    """bit b of x at bit step * b"""
    out = np.zeros_like(x)
    for b in range(bits):
        out |= ((x >> np.uint32(b)) & np.uint32(1)) << np.uint32(step * b)
    return out


def cells(rays, lo, scale):
    """(n, 3) uint32: the origin's cell per axis."""
    o = np.asarray(rays, F).reshape(-1, 6)[:, 0:3]
    with np.errstate(all="ignore"):
        t = (o - np.asarray(lo, F)) * np.asarray(scale, F)
        return np.fmin(np.fmax(t, F(0)), F((1 << CB) - 1)).astype(np.uint32)


def dir_cells(rays):
    """(n, 2) uint32: (u, v) of the octahedral map."""
    d = np.asarray(rays, F).reshape(-1, 6)[:, 3:6]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        a = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, py = dx / a, dy / a
        fx = (F(1) - np.abs(py)) * np.where(px < 0, F(-1), F(1))
        fy = (F(1) - np.abs(px)) * np.where(py < 0, F(-1), F(1))
        low = dz < 0
        qx, qy = np.where(low, fx, px).astype(F), np.where(low, fy, py).astype(F)
        cell = lambda q: np.fmin(np.fmax((q + F(1)) * F(1 << (DB - 1)), F(0)), F((1 << DB) - 1)).astype(np.uint32)
        return np.stack([cell(qx), cell(qy)], axis=1)


def keys(rays, lo, scale):
    """(n,) uint32 keys: cellMorton << 2 DB | dirMorton."""
    c, uv = cells(rays, lo, scale), dir_cells(rays)
    cm = _spread(c[:, 0], 3, CB) | _spread(c[:, 1], 3, CB) << np.uint32(1) | _spread(c[:, 2], 3, CB) << np.uint32(2)
    dm = _spread(uv[:, 0], 2, DB) | _spread(uv[:, 1], 2, DB) << np.uint32(1)
    return (cm << np.uint32(2 * DB) | dm).astype(np.uint32)


def order(k):
    """The coherent order of keys k: nondecreasing keys, equal keys in index order."""
    return np.argsort(k, kind="stable").astype(np.uint32)


def special_rays(lo=(-1.0, -2.0, -3.0), hi=(3.0, 2.0, 5.0)):
    """Rays on the key's edges, for a box [lo, hi]: zero, -0, NaN and infinite directions; NaN and infinite origins;
    origins outside the box and exactly on lo and hi; directions along each axis in both signs, and with dz = -0.0.
    (n, 6) float32."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    mid = ((lo + hi) * F(0.5)).astype(F)
    nan, inf = F(np.nan), F(np.inf)
    d0 = (0.3, -0.5, 0.8)
    rows = []
    for d in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (nan, 1.0, 1.0), (1.0, nan, -1.0), (1.0, 1.0, nan), (nan, nan, nan),
              (inf, 1.0, 1.0), (1.0, -inf, -1.0), (inf, inf, inf), (1.0, 2.0, -inf), (-inf, 0.0, 0.0)):
        rows.append(tuple(mid) + d)
    for o in ((nan, mid[1], mid[2]), (mid[0], nan, nan), (inf, mid[1], mid[2]), (mid[0], -inf, inf), (-inf, -inf, -inf),
              tuple(lo - F(10)), tuple(hi + F(10)), (lo[0] - F(1), mid[1], hi[2] + F(1)), tuple(lo), tuple(hi),
              (lo[0], hi[1], mid[2]), tuple(np.nextafter(hi, -inf)), tuple(np.nextafter(lo, -inf))):
        rows.append(tuple(o) + d0)
    for a in range(3):
        for s in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[a] = s
            rows.append(tuple(mid) + tuple(d))
    for d in ((1.0, 1.0, -0.0), (-1.0, 0.5, -0.0), (-0.0, -1.0, 0.0), (1.0, -0.0, -1.0), (-0.0, 1.0, -2.0)):
        rows.append(tuple(mid) + d)
    return np.array(rows, F)
