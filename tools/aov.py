#!/usr/bin/env python3
"""Depth, object-id and normal images of a scene from its camera (GPU box): the pinhole frame's primary rays through
one hit query (rfx.h rfx_query_hits) -- no shading, no random stream -- written as three TGA files.

    python tools/aov.py default out/aov [--size 640x480] [--layer K]

writes PREFIX_depth.tga (grey: near white, far black, scaled to the frame's own nearest and farthest hit; the sky
black), PREFIX_object.tga (a fixed colour per object index, the sky black) and PREFIX_normal.tga (the unit normal
mapped from [-1, 1] to [0, 255] per channel, the sky black).  --layer K: the images of what lies behind K hits of every
pixel's ray (Renderer.query_layers, rfx.h "Ray intervals"; 0, the default, is the first hit), a pixel whose ray has run out
of hits black.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reflaxman_amd import _lib, cameras, scenes  # noqa: E402
from reflaxman_amd.render import Renderer, build_scene  # noqa: E402


def pack(rgb8) -> np.ndarray:
    c = rgb8.astype(np.uint32)
    return np.ascontiguousarray(np.uint32(0xFF000000) | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", help="a scene name (reflaxman_amd.scenes) or a .scene file")
    ap.add_argument("prefix", help="the files written are PREFIX_depth.tga, PREFIX_object.tga, PREFIX_normal.tga")
    ap.add_argument("--size", default="640x480", help="WxH")
    ap.add_argument("--layer", type=int, default=0, help="the K-th hit behind the first (0: the first)")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))
    desc = scenes.parse_scene_file(args.scene) if os.path.isfile(args.scene) else scenes.get_scene(args.scene)
    scene, cam = build_scene(desc)
    r = Renderer()
    r.set_scene(scene)
    # rows bottom-up, as the renderer's images and rfx_tga_save's rows are; an 8x8 tile of the raster per wave
    rays = cameras.pinhole_rays(tuple(cam.eye), cam.view, cam.fov, W, H)
    if args.layer < 0:
        ap.error("--layer: 0 or more")
    want = ("object", "distance", "normal")
    out = r.query_layers(rays, args.layer + 1, want=want, raster_width=W)[args.layer] if args.layer else \
        r.query_hits(rays, raster_width=W, want=want)
    r.close()
    hit = out["object"] >= 0
    images = {}
    grey = np.zeros(W * H, np.float64)
    if hit.any():
        d = out["distance"][hit].astype(np.float64)
        grey[hit] = 1.0 - 0.9 * (d - d.min()) / max(d.max() - d.min(), 1e-30)
    images["depth"] = np.repeat((grey * 255.0).astype(np.uint8)[:, None], 3, axis=1)
    idx = out["object"].astype(np.uint32)  # a multiplicative hash: neighbouring indices get unlike colours
    h = (idx + np.uint32(1)) * np.uint32(2654435761)
    images["object"] = np.where(hit[:, None], np.stack([(h >> 24) | 64, ((h >> 16) & 255) | 64, ((h >> 8) & 255) | 64], axis=1), 0)
    nrm = out["normal"].astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    images["normal"] = np.where(hit[:, None], (nrm * 0.5 + 0.5) * 255.0, 0.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.prefix)), exist_ok=True)
    for what, img in images.items():
        path = f"{args.prefix}_{what}.tga"
        _lib.check(_lib.load().rfx_tga_save(os.fsencode(path), W, H, _lib.u32ptr(pack(img.astype(np.uint8).reshape(H, W, 3)))),
                   "rfx_tga_save")
    print(f"{args.prefix}_{{depth,object,normal}}.tga: {W}x{H} of {desc.name}, layer {args.layer}, {int(hit.sum())} of {W * H} pixels hit")


if __name__ == "__main__":
    main()
