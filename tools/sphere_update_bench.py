#!/usr/bin/env python3
"""Moving spheres (GPU box): what rfx_renderer_update_spheres costs against rfx_renderer_set_scene of the moved scene,
and what a frame costs on a refitted (stale) pair tree against a freshly built one -- ONE process on ONE GPU, the arms
alternating round by round (medians over the rounds), in the manner of tools/mesh_update_bench.py.

    python tools/sphere_update_bench.py --spheres 4096 [--rounds R] [--calls F] [--out DIR]
    python tools/sphere_update_bench.py --spheres 17600 ...

scenes.stress_scene(N): 4096 is C5, whose pair tree the bounce kernel stages in LDS; 4,400 spheres per pair of a leaf
(17,600 at the default leaf of four pairs) put the tree beyond the LDS, and the bounce kernel walks it in global memory.
The form that ran is in the record (bounce_form: 2 LDS, 1 global).

Update cost, per call:
    update_all      every sphere's centre and radius (device array, 4 floats a sphere), the chunk bounds and the whole
                    tree's refit: F calls between two device events, R rounds
    update_1pct     the same for 1% of the spheres by id (the refit is still the whole tree's)
    set_scene       rfx_renderer_set_scene of the host scene moved to the same spheres: a host clock around the call,
                    which ends synchronised; scene_edit is the host's rfx_scene_set_spheres before it
Trace cost after a refit, per move (jiggle: centres +- 0.3, radii x [0.8, 1.25]; shuffle: the centres permuted among
the spheres, so the topology cut at the old positions is stale everywhere):
    frame_refit     frames on a renderer that got the old scene and then the update
    frame_fresh     frames on a renderer whose set_scene got the moved scene
Before timing the two renderers' frames must be equal word for word from one stream state.  Frames are W x H, depth D
(--frame W H D), G frames between two device events (--frames G).  One JSON object goes to stdout and to
DIR/sphere_update_stress<N>.json (default profiles/r25).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reflaxman_amd import _lib, scenes  # noqa: E402
from reflaxman_amd.render import Renderer, build_scene, make_frame  # noqa: E402

SEED = 1350490027
F32 = np.float32


def spheres_of(desc):
    return np.array([[*ob[1], ob[2]] for ob in desc.objects if ob[0] == "sphere"], F32).reshape(-1, 4)


def move(S, kind):
    rng = np.random.default_rng(21)
    S = S.copy()
    if kind == "jiggle":
        S[:, :3] += rng.uniform(-0.3, 0.3, (len(S), 3)).astype(F32)
        S[:, 3] *= rng.uniform(0.8, 1.25, len(S)).astype(F32)
    else:
        S[:, :3] = S[rng.permutation(len(S)), :3]
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spheres", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40, help="update calls per timed window")
    ap.add_argument("--frames", type=int, default=4, help="frames per timed window")
    ap.add_argument("--frame", type=int, nargs=3, default=(1280, 720, 6), metavar=("W", "H", "D"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sphere_update_bench: needs a GPU (no CPU fallback)")
    L = _lib.load()
    desc = scenes.stress_scene(args.spheres)
    scene, cam = build_scene(desc)  # edited in place by the set_scene arm
    S0 = spheres_of(desc)
    n = len(S0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = C.c_void_p(stream.cuda_stream)
    W, H, D = args.frame
    frame = make_frame(cam, W, H, D, 1)
    img = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]

    def renderer():
        r = Renderer(sphere_seed=SEED, jitter_seed=0)
        r.set_stream(stream.cuda_stream)
        return r

    def window(fn, count):
        """device ms per call of `count` calls of fn enqueued back to back"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(count):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / count

    # ---- update cost against set_scene
    S1 = move(S0, "jiggle")
    d_s = [torch.from_numpy(S0).cuda(), torch.from_numpy(S1).cuda()]
    one = max(1, n // 100)
    ids = np.sort(np.random.default_rng(5).permutation(n)[:one]).astype(np.int32)
    d_ids = torch.from_numpy(ids).cuda()
    d_part = [torch.from_numpy(np.ascontiguousarray(S[ids])).cuda() for S in (S0, S1)]
    stream.synchronize()
    ru = renderer()
    ru.set_scene(scene)
    info = ru.accel_info()
    flip = [0]

    def upd_all():
        flip[0] ^= 1
        _lib.check(L.rfx_renderer_update_spheres(ru._h, 0, n, C.c_void_p(d_s[flip[0]].data_ptr()), None, sp))

    def upd_part():
        flip[0] ^= 1
        _lib.check(L.rfx_renderer_update_spheres(ru._h, 0, one, C.c_void_p(d_part[flip[0]].data_ptr()),
                                                 C.c_void_p(d_ids.data_ptr()), sp))

    rs = renderer()
    t = {"update_all": [], "update_1pct": [], "set_scene": [], "scene_edit": [], "set_scene_unmoved": []}
    for fn in (upd_all, upd_part):  # warm-up: code objects loaded, every shape once
        window(fn, 4)
    rs.set_scene(scene)
    for rnd in range(args.rounds):
        t["update_all"].append(window(upd_all, args.calls))
        t["update_1pct"].append(window(upd_part, args.calls))
        # set_scene without an edit before it (the scene as the last round left it) ...
        t0 = time.perf_counter()
        _lib.check(L.rfx_renderer_set_scene(rs._h, scene._h))  # synchronous: its uploads are blocking copies
        _lib.check(L.rfx_synchronize(rs._h))
        t1 = time.perf_counter()
        t["set_scene_unmoved"].append((t1 - t0) * 1e3)
        # ... and with rfx_scene_set_spheres before it
        v = S1 if rnd % 2 == 0 else S0
        t0 = time.perf_counter()
        _lib.check(L.rfx_scene_set_spheres(scene._h, 0, n, _lib.fptr(v)))
        t1 = time.perf_counter()
        _lib.check(L.rfx_renderer_set_scene(rs._h, scene._h))
        _lib.check(L.rfx_synchronize(rs._h))
        t2 = time.perf_counter()
        t["scene_edit"].append((t1 - t0) * 1e3)
        t["set_scene"].append((t2 - t1) * 1e3)
    out = {"scene": desc.name, "spheres": n, "sph_nodes": info.sph_nodes, "sph_depth": info.sph_depth,
           "rounds": args.rounds, "calls_per_window": args.calls, "update_calls_timed": args.rounds * args.calls,
           "ids_per_1pct_call": one, "frame": [W, H, D], "frames_per_window": args.frames,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()},
           "device_sha256": _lib.device_sha256()}
    out["set_scene_over_update_all"] = out["ms"]["set_scene"]["median"] / out["ms"]["update_all"]["median"]
    ru.close()
    rs.close()

    # ---- trace cost after a refit against a fresh build
    _lib.check(L.rfx_scene_set_spheres(scene._h, 0, n, _lib.fptr(S0)))
    out["trace"] = {}
    for kind in ("jiggle", "shuffle"):
        Sk = move(S0, kind)
        refit, fresh = renderer(), renderer()
        d_k = torch.from_numpy(Sk).cuda()
        stream.synchronize()
        _lib.check(L.rfx_renderer_set_scene(refit._h, scene._h))  # the old positions' tree
        _lib.check(L.rfx_renderer_update_spheres(refit._h, 0, n, C.c_void_p(d_k.data_ptr()), None, sp))
        _lib.check(L.rfx_scene_set_spheres(scene._h, 0, n, _lib.fptr(Sk)))
        _lib.check(L.rfx_renderer_set_scene(fresh._h, scene._h))
        _lib.check(L.rfx_scene_set_spheres(scene._h, 0, n, _lib.fptr(S0)))
        arms = {"frame_refit": (refit, img[0]), "frame_fresh": (fresh, img[1])}
        for r, buf in arms.values():
            r.set_rng(SEED, 0)
            r.render_frame(frame, buf.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        if not torch.equal(img[0], img[1]):
            sys.exit(f"sphere_update_bench: {kind}: the refitted renderer's frame differs from the fresh one's")
        tk = {k: [] for k in arms}
        for rnd in range(args.rounds):
            for k in (list(arms)[rnd % 2:] + list(arms)[:rnd % 2]):
                r, buf = arms[k]
                tk[k].append(window(lambda: r.render_frame(frame, buf.data_ptr(), stream=stream.cuda_stream), args.frames))
        out["trace"][kind] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in tk.items()}
        out["trace"][kind]["refit_over_fresh"] = (out["trace"][kind]["frame_refit"]["median"] /
                                                  out["trace"][kind]["frame_fresh"]["median"])
        out["trace"][kind]["bounce_form"] = {k: r.bounce_form() for k, (r, _) in arms.items()}
        refit.close()
        fresh.close()
    os.makedirs(args.out, exist_ok=True)
    print(json.dumps(out))
    with open(os.path.join(args.out, f"sphere_update_{desc.name}.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
