"""Ray generators for Renderer.trace_rays (rfx.h rfx_trace_rays): (n, 6) float32 records, origin then direction.

``pinhole_rays`` is the reference's own camera (Render.cpp:146-156, 184-185) in float32, operation for operation, so
tracing its rays reproduces a one-sample non-additive frame bit for bit; ``equirect_rays`` is a camera the reference's
pixel loop cannot express.  Rows run bottom-up like the renderer's images (row 0 = bottom), so a batch traced with
``raster_width=W`` is a W x H image that ``rfx_tga_save`` writes as it stands.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util

import numpy as np

f32 = np.float32


def camera_rz(width: int, fov: float) -> np.float32:
    """rz = W / 2 / tanf(fov / 2) (Render.cpp:148): the library's rfx_camera_rz, or -- no library loaded -- the same
    three float operations on libm's tanf."""
    from . import _lib
    if _lib._lib is not None:
        return f32(_lib._lib.rfx_camera_rz(int(width), float(f32(fov))))
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.tanf.restype, m.tanf.argtypes = C.c_float, [C.c_float]
    return f32(f32(f32(width) / f32(2.0)) / f32(m.tanf(C.c_float(f32(fov) / f32(2.0)))))


def _records(origin, dirs) -> np.ndarray:
    out = np.empty((dirs.shape[0], 6), np.float32)
    out[:, 0:3] = np.asarray(origin, np.float32).reshape(1, 3)
    out[:, 3:6] = dirs
    return out


def pinhole_rays(eye, view, fov: float, W: int, H: int) -> np.ndarray:
    """The rays of Render::renderNext's pixel loop with sampleNum 1 and no jitter, in raster order (pixel y W + x):
    ray = view (x - W/2, y - H/2, rz), every product and sum in float32 and in the reference's order,
    (m11 x + m12 y) + m13 z (Matrix33 * Vector3)."""
    m = np.asarray(view, np.float32).reshape(3, 3)
    rz = camera_rz(W, fov)
    wh, hh = f32(W) / f32(2.0), f32(H) / f32(2.0)                            # Render.cpp:149-150
    x = np.arange(W, dtype=np.float32)[None, :] - wh                        # Render.cpp:152-153; + 0 + 0 changes nothing
    y = np.arange(H, dtype=np.float32)[:, None] - hh
    x, y = np.broadcast_to(x, (H, W)).reshape(-1), np.broadcast_to(y, (H, W)).reshape(-1)
    d = np.empty((W * H, 3), np.float32)
    for k in range(3):
        d[:, k] = (x * m[k, 0] + y * m[k, 1]) + rz * m[k, 2]
    return _records(eye, d)


def pinhole_ray(eye, view, fov: float, W: int, H: int, x: int, y: int) -> np.ndarray:
    """The one record of ``pinhole_rays`` for pixel (x, y) (row 0 = bottom), by the same float32 operations: what a
    pick under that pixel traces (Render.pick)."""
    m = np.asarray(view, np.float32).reshape(3, 3)
    rz = camera_rz(W, fov)
    fx, fy = f32(x) - f32(W) / f32(2.0), f32(y) - f32(H) / f32(2.0)
    d = np.array([[(fx * m[k, 0] + fy * m[k, 1]) + rz * m[k, 2] for k in range(3)]], np.float32)
    return _records(eye, d)[0]


def equirect_rays(eye, W: int, H: int) -> np.ndarray:
    """A 360 x 180 degree panorama from ``eye``: column x looks at longitude (x + 1/2) / W of a turn, measured from +z
    towards +x, row y (row 0 = bottom) at latitude ((y + 1/2) / H - 1/2) pi; unit directions, pixel centres, so no ray
    points exactly at a pole and the first and last columns sit half a pixel either side of the -z seam."""
    lon = (np.arange(W, dtype=np.float64) + 0.5) / W * 2.0 * np.pi - np.pi
    lat = ((np.arange(H, dtype=np.float64) + 0.5) / H - 0.5) * np.pi
    cl = np.cos(lat)[:, None]
    d = np.stack([np.broadcast_to(cl * np.sin(lon)[None, :], (H, W)),
                  np.broadcast_to(np.sin(lat)[:, None], (H, W)),
                  np.broadcast_to(cl * np.cos(lon)[None, :], (H, W))], axis=-1)
    return _records(eye, d.reshape(-1, 3).astype(np.float32))
