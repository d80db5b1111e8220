#!/usr/bin/env python3
"""Moving meshes (GPU box): what rfx_renderer_update_triangles and rfx_renderer_recut_triangles cost against
rfx_renderer_set_scene of the moved scene, and what a frame costs on a refitted (stale) tree, on a re-cut tree and on a
freshly built one -- ONE process on ONE GPU, the arms alternating round by round (medians over the rounds), in the
manner of tools/hits_bench.py.

    python tools/mesh_update_bench.py --scene mesh40x32 [--rounds R] [--calls F] [--out DIR]
    python tools/mesh_update_bench.py --scene soup100000 ...

mesh40x32: scenes.mesh_scene(40, 32), 2,560 triangles under the 8 default spheres; soup100000: the 100,000 triangles of
scenes.soup_scene(100000) as one mesh of one material (the timing reads no material).  Both with the triangle BVH
(rfx_renderer_set_tri_accel 1).

Update cost, per call:
    update_all      the whole mesh's vertices (device array, 9 floats a triangle) and the whole tree's refit: F calls
                    between two device events, R rounds (R F >= 200 calls)
    update_1pct     the same for a range of 1% of the triangles (the refit is still the whole tree's)
    recut           rfx_renderer_recut_triangles at the vertices the last update left: keys, sort, leaf records,
                    topology and the whole tree's refit, timed the same way
    set_scene       rfx_renderer_set_scene of the host scene moved to the same vertices: a host clock around the call,
                    which ends synchronised -- the only way to move a mesh before this entry point; scene_edit is the
                    host's rfx_scene_set_triangle_vertices before it
Trace cost after a refit, per deformation (wave: every vertex on a height wave of amplitude 0.1; shuffle: every triangle
moved by up to +-6 units on each axis, so the topology cut at the old positions is stale):
    frame_refit     frames on a renderer that got the old scene and then the update: the stale tree
    frame_recut     ... and then the re-cut
    frame_fresh     frames on a renderer whose set_scene got the moved scene
Before timing the three renderers' frames must be equal word for word from one stream state.  Frames are W x H, depth D
(--frame W H D), G frames between two device events (--frames G).  Beside each arm's time goes its tree's quality, a
surface-area figure computed here from rfx_renderer_tri_bvh_nodes: the sum of every finite child box's area over the
root box's area (the expected number of boxes a random line through the root meets; lower is better).  One JSON object
goes to stdout and to DIR/mesh_update_<scene>.json (default profiles/r23).
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
from reflaxman_amd.render import Camera, Color, Material, Renderer, Scene, Vector3, build_scene, make_frame  # noqa: E402

SEED = 1350490027
F32 = np.float32


def vertices_of(desc):
    return np.array([[ob[1], ob[2], ob[3]] for ob in desc.objects if ob[0] == "triangle"], F32)


def make_scene(name):
    """(Scene, Camera, vertices) -- the Scene is edited in place by the set_scene arm"""
    if name == "mesh40x32":
        desc = scenes.mesh_scene(40, 32)
        s, cam = build_scene(desc)
        return s, cam, vertices_of(desc)
    desc = scenes.soup_scene(100000)
    V = vertices_of(desc)
    s = Scene(Color(*desc.diffuse[:3]), desc.diffuse[3])
    for (o, r, c, p) in desc.lights:
        s.addLight(Vector3(*o), r, Color(*c), p)
    s.addMesh(V.reshape(-1, 3), np.arange(3 * len(V), dtype=np.uint32).reshape(-1, 3),
              Material(_lib.METAL, Color(0.8, 0.7, 0.6), 0.4, 0.0))
    eye, at, fov = desc.camera
    return s, Camera(Vector3(*eye), Vector3(*at), fov), V


def deform(V, kind):
    V = V.copy()
    if kind == "wave":
        V[..., 1] += (0.1 * np.sin(0.9 * V[..., 0].astype(np.float64) + 0.7 * V[..., 2])).astype(F32)
    else:
        V += np.random.default_rng(21).uniform(-6.0, 6.0, (len(V), 1, 3)).astype(F32)
    return V


def sah(nodes):
    """sum of the finite child boxes' areas over the area of the root box -- the union of the finite boxes: a tree with
    an ill triangle under each child of the root has no finite box at the top -- and how many child boxes are all of
    space (NaN), which the sum leaves out though every ray descends through them"""
    boxes = nodes[0].astype(np.float64).reshape(-1, 6)
    finite = np.isfinite(boxes).all(axis=1)
    boxes = boxes[finite]
    d = boxes[:, 3:] - boxes[:, :3]
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    r = boxes[:, 3:].max(axis=0) - boxes[:, :3].min(axis=0)
    return {"sah": float(area.sum() / (r[0] * r[1] + r[1] * r[2] + r[2] * r[0])), "all_space_boxes": int((~finite).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("mesh40x32", "soup100000"), default="mesh40x32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40, help="update calls per timed window")
    ap.add_argument("--frames", type=int, default=4, help="frames per timed window")
    ap.add_argument("--frame", type=int, nargs=3, default=(1280, 720, 6), metavar=("W", "H", "D"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_update_bench: needs a GPU (no CPU fallback)")
    L = _lib.load()
    scene, cam, V0 = make_scene(args.scene)
    n = len(V0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = C.c_void_p(stream.cuda_stream)
    W, H, D = args.frame
    frame = make_frame(cam, W, H, D, 1)
    img = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(3)]

    def renderer():
        r = Renderer(sphere_seed=SEED, jitter_seed=0)
        r.set_stream(stream.cuda_stream)
        r.set_tri_accel(1)
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
    V1 = deform(V0, "wave")
    d_v = [torch.from_numpy(V0).cuda(), torch.from_numpy(V1).cuda()]
    stream.synchronize()
    ru = renderer()
    ru.set_scene(scene)
    info = ru.accel_info()
    one = max(1, n // 100)
    flip = [0]

    def upd_all():
        flip[0] ^= 1
        _lib.check(L.rfx_renderer_update_triangles(ru._h, 0, n, C.c_void_p(d_v[flip[0]].data_ptr()), 3 * n, None, sp))

    def upd_part():
        flip[0] ^= 1
        _lib.check(L.rfx_renderer_update_triangles(ru._h, n // 2, one, C.c_void_p(d_v[flip[0]].data_ptr() + 36 * (n // 2)),
                                                   3 * one, None, sp))

    def recut():
        _lib.check(L.rfx_renderer_recut_triangles(ru._h, sp))

    rs = renderer()
    t = {"update_all": [], "update_1pct": [], "recut": [], "set_scene": [], "scene_edit": []}
    for fn in (upd_all, upd_part, recut):  # warm-up: code objects loaded, every shape once
        window(fn, 4)
    rs.set_scene(scene)
    for rnd in range(args.rounds):
        t["update_all"].append(window(upd_all, args.calls))
        t["update_1pct"].append(window(upd_part, args.calls))
        t["recut"].append(window(recut, args.calls))
        v = V1 if rnd % 2 == 0 else V0
        t0 = time.perf_counter()
        _lib.check(L.rfx_scene_set_triangle_vertices(scene._h, 0, n, _lib.fptr(v)))
        t1 = time.perf_counter()
        _lib.check(L.rfx_renderer_set_scene(rs._h, scene._h))  # synchronous: its uploads are blocking copies
        _lib.check(L.rfx_synchronize(rs._h))
        t2 = time.perf_counter()
        t["scene_edit"].append((t1 - t0) * 1e3)
        t["set_scene"].append((t2 - t1) * 1e3)
    out = {"scene": args.scene, "triangles": n, "tri_nodes": info.tri_nodes, "tri_depth": info.tri_depth,
           "tri_residual": info.tri_residual, "rounds": args.rounds, "calls_per_window": args.calls,
           "update_calls_timed": args.rounds * args.calls, "frame": [W, H, D], "frames_per_window": args.frames,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()},
           "device_sha256": _lib.device_sha256()}
    out["set_scene_over_update_all"] = out["ms"]["set_scene"]["median"] / out["ms"]["update_all"]["median"]
    out["set_scene_over_recut"] = out["ms"]["set_scene"]["median"] / out["ms"]["recut"]["median"]
    ru.close()
    rs.close()

    # ---- trace cost after a refit against a fresh build
    _lib.check(L.rfx_scene_set_triangle_vertices(scene._h, 0, n, _lib.fptr(V0)))
    out["trace"] = {}
    for kind in ("wave", "shuffle"):
        Vk = deform(V0, kind)
        refit, cut, fresh = renderer(), renderer(), renderer()
        d_k = torch.from_numpy(Vk).cuda()
        stream.synchronize()
        for r in (refit, cut):
            _lib.check(L.rfx_renderer_set_scene(r._h, scene._h))  # the old positions' tree
            _lib.check(L.rfx_renderer_update_triangles(r._h, 0, n, C.c_void_p(d_k.data_ptr()), 3 * n, None, sp))
        _lib.check(L.rfx_renderer_recut_triangles(cut._h, sp))
        _lib.check(L.rfx_scene_set_triangle_vertices(scene._h, 0, n, _lib.fptr(Vk)))
        _lib.check(L.rfx_renderer_set_scene(fresh._h, scene._h))
        _lib.check(L.rfx_scene_set_triangle_vertices(scene._h, 0, n, _lib.fptr(V0)))
        arms = {"frame_refit": (refit, img[0]), "frame_recut": (cut, img[1]), "frame_fresh": (fresh, img[2])}
        for r, buf in arms.values():
            r.set_rng(SEED, 0)
            r.render_frame(frame, buf.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        if not (torch.equal(img[0], img[2]) and torch.equal(img[1], img[2])):
            sys.exit(f"mesh_update_bench: {kind}: the refitted or the re-cut renderer's frame differs from the fresh one's")
        tk = {k: [] for k in arms}
        for rnd in range(args.rounds):
            for k in (list(arms)[rnd % 3:] + list(arms)[:rnd % 3]):
                r, buf = arms[k]
                tk[k].append(window(lambda: r.render_frame(frame, buf.data_ptr(), stream=stream.cuda_stream), args.frames))
        out["trace"][kind] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in tk.items()}
        out["trace"][kind]["refit_over_fresh"] = (out["trace"][kind]["frame_refit"]["median"] /
                                                  out["trace"][kind]["frame_fresh"]["median"])
        out["trace"][kind]["recut_over_fresh"] = (out["trace"][kind]["frame_recut"]["median"] /
                                                  out["trace"][kind]["frame_fresh"]["median"])
        out["trace"][kind]["refit_over_recut"] = (out["trace"][kind]["frame_refit"]["median"] /
                                                  out["trace"][kind]["frame_recut"]["median"])
        out["trace"][kind]["fresh_residual"] = fresh.accel_info().tri_residual
        out["trace"][kind]["sah"] = {k: sah(r.tri_bvh_nodes()) for k, (r, _) in arms.items()}
        out["trace"][kind]["tri_depth"] = {k: r.accel_info().tri_depth for k, (r, _) in arms.items()}
        refit.close()
        cut.close()
        fresh.close()
    os.makedirs(args.out, exist_ok=True)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out, f"mesh_update_{args.scene}.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
