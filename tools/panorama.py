#!/usr/bin/env python3
"""A 360 x 180 degree panorama of a scene from its camera's eye point (GPU box): cameras.equirect_rays traced as one
ray batch (rfx.h rfx_trace_rays) -- a view Render::renderNext's pinhole loop cannot produce -- written as a TGA.

    python tools/panorama.py synth16_sky pano.tga [--width 2048] [--depth 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reflaxman_amd import _lib, cameras, scenes  # noqa: E402
from reflaxman_amd.render import Renderer, build_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", help="a scene name (reflaxman_amd.scenes) or a .scene file")
    ap.add_argument("out", help="the TGA file to write")
    ap.add_argument("--width", type=int, default=2048, help="image width; the height is half of it")
    ap.add_argument("--depth", type=int, default=8)
    args = ap.parse_args()
    desc = scenes.parse_scene_file(args.scene) if os.path.isfile(args.scene) else scenes.get_scene(args.scene)
    W, H = args.width, max(1, args.width // 2)
    scene, cam = build_scene(desc)
    r = Renderer()
    r.set_scene(scene)
    # rows bottom-up, as the renderer's images and rfx_tga_save's rows are; an 8x8 tile of the raster per wave
    _, argb = r.trace_rays(cameras.equirect_rays(tuple(cam.eye), W, H), args.depth, raster_width=W, argb=True)
    argb = np.ascontiguousarray(argb | np.uint32(0xFF000000))
    _lib.check(_lib.load().rfx_tga_save(os.fsencode(args.out), W, H, _lib.u32ptr(argb)), "rfx_tga_save")
    r.close()
    print(f"{args.out}: {W}x{H} panorama of {desc.name}, depth {args.depth}")


if __name__ == "__main__":
    main()
