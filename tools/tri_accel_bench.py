#!/usr/bin/env python3
"""Triangle-BVH timing (GPU): trace ms and Mrays/s of rfx_renderer_set_tri_accel modes on mesh scenes, interleaved in
one process, every mode's frame checked equal to mode 0's before its timing counts.

    python tools/tri_accel_bench.py --scenes soup64,soup128,soup256 [--modes 0,1] [--libs base,notribvh]
                                    [--width 1920 --height 1080 --depth 8 --frames 3 --rounds 3] [--out FILE]

Scenes are reflaxman_amd.scenes.get_scene names (soup<n>, soup<n>_s<spheres>, mesh<nx>x<nz>).  --libs: variant builds
of tools/ab.py (reflaxman_amd/lib/variants) instead of the product library; a build without the triangle walkers
(notribvh) runs the same kernels in either mode.  One JSON line per (scene, library, mode); --out appends them.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ab  # noqa: E402
from reflaxman_amd import _build, _lib, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", required=True)
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--libs", default="")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    libs = [("product", _build.LIB)] if not args.libs else [
        (n, os.path.join(_build.LIBDIR, "variants", f"librfx_{n}.so")) for n in args.libs.split(",")]
    modes = [int(m) for m in args.modes.split(",")]
    W, H = args.width, args.height
    for name in args.scenes.split(","):
        desc = scenes.get_scene(name)
        runners = [ab.Runner(f"{ln}@tri{m}", path, desc, W, H, args.depth, 1350490027, tri_accel=m)
                   for ln, path in libs for m in modes]
        infos = []
        for r in runners:
            a = _lib.AccelInfo()
            assert r.L.rfx_renderer_accel_info(r.r, a) == 0
            infos.append(a)
        first = [r.frame_hashes(1) for r in runners]
        for r in runners:
            r.render(args.warmup)
        times = {r.name: [] for r in runners}
        for _ in range(args.rounds):
            for r in runners:
                times[r.name].append(r.timed(args.frames)[1])
        base = statistics.median(times[runners[0].name])
        for r, a, h in zip(runners, infos, first):
            med = statistics.median(times[r.name])
            rec = {"scene": name, "triangles": desc.n_triangles, "spheres": desc.n_spheres, "run": r.name,
                   "width": W, "height": H, "depth": args.depth, "tri_nodes": a.tri_nodes, "tri_depth": a.tri_depth,
                   "leaf": a.tri_leaf_size, "residual": a.tri_residual, "narrow_tri_bvh": a.narrow_tri_bvh,
                   "frame_equals_first_run": h == first[0], "trace_ms_median": round(med, 4),
                   "trace_ms_min": round(min(times[r.name]), 4), "vs_first": round(med / base, 4),
                   "mrays_trace_only": round(W * H / (med * 1e-3) / 1e6, 1)}
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        for r in runners:
            r.close()


if __name__ == "__main__":
    main()
