#!/usr/bin/env python3
"""Hit queries against a depth-1 ray batch (GPU box): rfx_query_hits / rfx_query_occluded on a frame's own primary
rays, interleaved with rfx_trace_rays at reflect_num 1 in ONE process on ONE GPU, in the manner of tools/rays_bench.py.

    python tools/hits_bench.py --config c3 [--rounds R] [--calls F] [--out DIR]
    python tools/hits_bench.py --config c5 ...

c3: synth16 3840x2160; c5: stress4096 3840x2160.  The rays are cameras.pinhole_rays of the scene's camera.  Before
anything is timed, the object plane's miss count must equal the number of pixels whose depth-1 colour (rfx_trace_rays)
is the sky's (sky_pixels below); the any-hit must count the remaining pixels, and the raster and permuted batches must
give the linear batch's objects.

Arms (every one its own renderer on the same scene and stream; a round times F calls of each arm in turn between two
device events; medians over the rounds):
    trace_d1, trace_d1_again   rfx_trace_rays at reflect_num 1, raster -- what a caller had for this question before,
                               pre-pass included; twice, so the pair's difference is the run's own noise band
    hits_raster / hits_linear / hits_permuted   rfx_query_hits, all six planes (56 B out per ray): raster_width = W,
                               0, and 0 on a fixed random permutation of the rays
    hits_object                rfx_query_hits, the object plane alone (4 B out per ray), raster
    occluded                   rfx_query_occluded, nothing left out, raster
    hits_permuted_order        rfx_rays_order alone on the permuted rays: the sort an incoherent caller would add
    hits_permuted_ordered      rfx_query_hits_ordered on the permuted rays with that order computed beforehand, all six
                               planes; hits_permuted_sum (no arm, the two medians added) is what stands against
                               hits_permuted, with hits_raster as the ceiling.  Before timing the ordered call's six
                               planes must equal the permuted arm's
    hits_permuted_object / hits_permuted_ordered_object   the same pair asking for the object plane alone: what the
                               ordered call's scattered stores cost (it writes each ray's words where the ray lies in
                               the caller's arrays, not where its wave runs)
One JSON line per arm goes to stdout and to DIR/hits_<config>.jsonl (default profiles/r13).

--span: the span queries' arms instead (rfx.h "Ray intervals"), by the same method, to DIR/span_<config>.jsonl:
    hits, hits_again           rfx_query_hits, all six planes, raster; twice: the pair is the run's noise band
    hits_span_none             rfx_query_hits_span without ends, the same planes: what carrying the span costs
    occluded, occluded_span_none   the same pair for the any-hit
    seg<f>_span / seg<f>_workaround   segment visibility with hi = f x the depth-1 hit distance (f = 0.5: nothing in the
                               way, f = 2: the first hit in the way): rfx_query_occluded_span with d_hi, against
                               rfx_query_hits' distance plane alone followed by a device compare with hi; `occluded` is the
                               unbounded any-hit beside them.  Before timing the two must agree on every ray
    layers4 / hits_x4          Renderer.query_layers(rays, 4) (object and distance; its stepping included) against four
                               plain rfx_query_hits calls for the same two planes
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reflaxman_amd import _lib, cameras, scenes  # noqa: E402
from reflaxman_amd.render import Renderer, build_scene  # noqa: E402

CONFIGS = {"c3": ("synth16", 3840, 2160), "c5": ("stress4096", 3840, 2160)}
SEED = 1350490027
PLANES = ("object", "distance", "point", "normal", "reflected", "colour")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c3")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13"))
    ap.add_argument("--span", action="store_true", help="the span queries' arms (see above)")
    args = ap.parse_args()
    if args.span:
        return span_main(args)
    import torch
    name, W, H = CONFIGS[args.config]
    desc = scenes.get_scene(name)
    scene, cam = build_scene(desc)
    n = W * H
    host_rays = cameras.pinhole_rays(tuple(cam.eye), cam.view, cam.fov, W, H)
    dirs = np.ascontiguousarray(host_rays[:, 3:6])
    perm = np.random.default_rng(12).permutation(n)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rays = torch.from_numpy(host_rays).cuda()
    rays_perm = torch.from_numpy(host_rays[perm]).cuda()
    del host_rays
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    out = {k: torch.zeros((n,) if k in ("object", "distance") else (n, 3),
                          dtype=torch.int32 if k == "object" else torch.float32, device="cuda") for k in PLANES}
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    L = _lib.load()
    sp = C.c_void_p(stream.cuda_stream)

    def renderer():
        r = Renderer(sphere_seed=SEED, jitter_seed=0)
        r.set_stream(stream.cuda_stream)
        r.set_scene(scene)
        return r

    def trace_arm():
        r = renderer()
        return r, lambda: _lib.check(L.rfx_trace_rays(r._h, C.c_void_p(rays.data_ptr()), n, 1, W,
                                                      C.c_void_p(rgb.data_ptr()), None, None, sp), "rfx_trace_rays")

    def hits_arm(src, rw, want):
        r = renderer()
        hp = _lib.HitPlanes(**{k: out[k].data_ptr() for k in want})
        return r, lambda: _lib.check(L.rfx_query_hits(r._h, C.c_void_p(src.data_ptr()), n, rw, C.byref(hp), sp),
                                     "rfx_query_hits")

    def occ_arm():
        r = renderer()
        return r, lambda: _lib.check(L.rfx_query_occluded(r._h, C.c_void_p(rays.data_ptr()), None, n, W,
                                                          C.c_void_p(occ.data_ptr()), sp), "rfx_query_occluded")

    order = torch.zeros(n, dtype=torch.int32, device="cuda")

    def order_arm():
        r = renderer()
        return r, lambda: _lib.check(L.rfx_rays_order(r._h, C.c_void_p(rays_perm.data_ptr()), n,
                                                      C.c_void_p(order.data_ptr()), None, sp), "rfx_rays_order")

    def ordered_arm(want):
        r = renderer()
        hp = _lib.HitPlanes(**{k: out[k].data_ptr() for k in want})
        return r, lambda: _lib.check(L.rfx_query_hits_ordered(r._h, C.c_void_p(rays_perm.data_ptr()),
                                                              C.c_void_p(order.data_ptr()), n, C.byref(hp), sp),
                                     "rfx_query_hits_ordered")

    arms = [("trace_d1", trace_arm(), 12), ("hits_raster", hits_arm(rays, W, PLANES), 56),
            ("hits_linear", hits_arm(rays, 0, PLANES), 56), ("hits_permuted", hits_arm(rays_perm, 0, PLANES), 56),
            ("hits_object", hits_arm(rays, W, ("object",)), 4), ("occluded", occ_arm(), 1),
            ("hits_permuted_order", order_arm(), 4), ("hits_permuted_ordered", ordered_arm(PLANES), 56),
            ("hits_permuted_object", hits_arm(rays_perm, 0, ("object",)), 4),
            ("hits_permuted_ordered_object", ordered_arm(("object",)), 4),
            ("trace_d1_again", trace_arm(), 12)]

    # the check before timing: misses of the object plane = sky-coloured pixels of the depth-1 frame; with it, the
    # any-hit of the same rays counts the hits, and the permuted batch is the linear one, permuted
    by = {a: rc for a, rc, _ in arms}
    for a in ("trace_d1", "hits_linear", "occluded"):
        by[a][1]()
    stream.synchronize()
    lin_obj = out["object"].clone()
    misses = int((lin_obj < 0).sum())
    occluded_n = int(occ.sum())
    sky = sky_pixels(by["trace_d1"][0], desc, dirs, rgb.cpu().numpy())
    by["hits_permuted"][1]()
    stream.synchronize()
    perm_ok = bool(torch.equal(out["object"], lin_obj[torch.from_numpy(perm).cuda()]))
    # the ordered call on the permuted rays, in the library's order: every word of the permuted arm's six planes
    perm_out = {k: out[k].clone() for k in PLANES}
    for k in PLANES:
        out[k].zero_()
    by["hits_permuted_order"][1]()
    by["hits_permuted_ordered"][1]()
    stream.synchronize()
    bits = lambda t: t.view(torch.int32)
    ordered_ok = all(bool(torch.equal(bits(out[k]), bits(perm_out[k]))) for k in PLANES)
    sorted_ok = bool(torch.equal(torch.sort(order.to(torch.int64)).values, torch.arange(n, device="cuda")))
    del perm_out
    by["hits_object"][1]()
    stream.synchronize()
    raster_ok = bool(torch.equal(out["object"], lin_obj))
    check = {"misses": misses, "sky_pixels": sky, "occluded": occluded_n, "permuted_equal": perm_ok,
             "raster_equal": raster_ok, "ordered_equal": ordered_ok, "order_is_a_permutation": sorted_ok}
    if misses != sky or n - misses != occluded_n or not (perm_ok and raster_ok and ordered_ok and sorted_ok):
        raise SystemExit(f"hits_bench: the check before timing failed: {check}")

    for arm, (r, call), _ in arms:
        for _ in range(3):
            call()
    stream.synchronize()
    ms = {arm: [] for arm, _, _ in arms}
    for _ in range(args.rounds):
        for arm, (r, call), _ in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                call()
            e1.record(stream)
            e1.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / args.calls)
    base = statistics.median(ms["trace_d1"])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"hits_{args.config}.jsonl"), "w") as f:
        for arm, (r, call), nbytes in arms:
            med = statistics.median(ms[arm])
            line = json.dumps({"config": args.config, "scene": name, "W": W, "H": H, "arm": arm, "rounds": args.rounds,
                               "calls_per_window": args.calls, "out_bytes_per_ray": nbytes, "check": check,
                               "ms_median": round(med, 4), "ms_min": round(min(ms[arm]), 4),
                               "ms_max": round(max(ms[arm]), 4), "mrays_s": round(n / med / 1e3, 1),
                               "vs_trace_d1": round(med / base, 4)})
            print(line)
            f.write(line + "\n")
            r.close()
        med = statistics.median(ms["hits_permuted_order"]) + statistics.median(ms["hits_permuted_ordered"])
        line = json.dumps({"config": args.config, "scene": name, "W": W, "H": H, "arm": "hits_permuted_sum",
                           "of": ["hits_permuted_order", "hits_permuted_ordered"], "ms_median": round(med, 4),
                           "mrays_s": round(n / med / 1e3, 1), "vs_trace_d1": round(med / base, 4),
                           "vs_hits_permuted": round(med / statistics.median(ms["hits_permuted"]), 4),
                           "vs_hits_raster": round(med / statistics.median(ms["hits_raster"]), 4)})
        print(line)
        f.write(line + "\n")


def span_main(args):
    import torch
    name, W, H = CONFIGS[args.config]
    scene, cam = build_scene(scenes.get_scene(name))
    n = W * H
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rays = torch.from_numpy(cameras.pinhole_rays(tuple(cam.eye), cam.view, cam.fov, W, H)).cuda()
    planes = lambda: {k: torch.zeros((n,) if k in ("object", "distance") else (n, 3),
                                     dtype=torch.int32 if k == "object" else torch.float32, device="cuda") for k in PLANES}
    out, out2 = planes(), planes()
    occ, occ2 = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2))
    L = _lib.load()
    sp = C.c_void_p(stream.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def renderer():
        r = Renderer(sphere_seed=SEED, jitter_seed=0)
        r.set_stream(stream.cuda_stream)
        r.set_scene(scene)
        return r

    def hits_arm(dst, want, span=False, times=1):
        r = renderer()
        hp = _lib.HitPlanes(**{k: dst[k].data_ptr() for k in want})

        def call():
            for _ in range(times):
                if span:
                    _lib.check(L.rfx_query_hits_span(r._h, p(rays), None, n, W, C.byref(hp), sp), "rfx_query_hits_span")
                else:
                    _lib.check(L.rfx_query_hits(r._h, p(rays), n, W, C.byref(hp), sp), "rfx_query_hits")
        return r, call

    def occ_arm(dst, hi=None, span=False):
        r = renderer()
        rs = _lib.RaySpan(d_hi=hi.data_ptr()) if hi is not None else None

        def call():
            if span:
                _lib.check(L.rfx_query_occluded_span(r._h, p(rays), None, C.byref(rs) if rs else None, n, W, p(dst), sp),
                           "rfx_query_occluded_span")
            else:
                _lib.check(L.rfx_query_occluded(r._h, p(rays), None, n, W, p(dst), sp), "rfx_query_occluded")
        return r, call

    def workaround_arm(dst, hi):
        r, q = hits_arm(out2, ("distance",))

        def call():
            q()
            torch.le(out2["distance"], hi, out=dst)
        return r, call

    def layers_arm():
        r = renderer()
        return r, lambda: r.query_layers(rays, 4, want=("object", "distance"), raster_width=W)

    # the depth-1 distances the segments are cut from
    r0, first = hits_arm(out, PLANES)
    first()
    stream.synchronize()
    dist = out["distance"].clone()
    ref = {k: out[k].clone() for k in PLANES}
    # (a ray that hits nothing gets a segment of length 1: nothing lies on it, and the workaround's FLT_MAX says so too)
    his = {f: torch.where(ref["object"] >= 0, dist * f, torch.ones_like(dist)) for f in (0.5, 2.0)}
    seg_occ = {f: torch.zeros(n, dtype=torch.bool, device="cuda") for f in his}
    arms = [("hits", (r0, first)), ("hits_span_none", hits_arm(out2, PLANES, span=True)), ("occluded", occ_arm(occ)),
            ("occluded_span_none", occ_arm(occ2, span=True))]
    for f, hi in his.items():
        arms += [(f"seg{f}_span", occ_arm(occ2, hi, span=True)), (f"seg{f}_workaround", workaround_arm(seg_occ[f], hi))]
    arms += [("layers4", layers_arm()), ("hits_x4", hits_arm(out2, ("object", "distance"), times=4)),
             ("hits_again", hits_arm(out, PLANES))]
    by = dict(arms)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    # the checks before timing
    by["hits_span_none"][1]()
    by["occluded"][1]()
    stream.synchronize()
    check = {"span_none_equal": all(bool(torch.equal(bits(out2[k]), bits(ref[k]))) for k in PLANES)}
    by["occluded_span_none"][1]()
    stream.synchronize()
    check["occluded_span_none_equal"] = bool(torch.equal(occ, occ2))
    check["occluded"] = int(occ.sum())
    for f in his:
        by[f"seg{f}_span"][1]()
        by[f"seg{f}_workaround"][1]()
        stream.synchronize()
        check[f"seg{f}_occluded"] = int(occ2.sum())
        check[f"seg{f}_equal"] = bool(torch.equal(occ2.bool(), seg_occ[f]))
    lay = by["layers4"][1]()
    stream.synchronize()
    check["layers_hit"] = [int((l["object"] >= 0).sum()) for l in lay]
    check["layer0_equal"] = bool(torch.equal(lay[0]["object"], ref["object"]))
    if not all(v for k, v in check.items() if k.endswith("equal")):
        raise SystemExit(f"hits_bench --span: the check before timing failed: {check}")
    for arm, (r, call) in arms:
        for _ in range(3):
            call()
    stream.synchronize()
    ms = {arm: [] for arm, _ in arms}
    for _ in range(args.rounds):
        for arm, (r, call) in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.calls):
                call()
            e1.record(stream)
            e1.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / args.calls)
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    against = {"hits_span_none": "hits", "hits_again": "hits", "occluded_span_none": "occluded", "layers4": "hits_x4"}
    for f in his:
        against[f"seg{f}_span"] = f"seg{f}_workaround"
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"span_{args.config}.jsonl"), "w") as fh:
        for arm, (r, call) in arms:
            rec = {"config": args.config, "scene": name, "W": W, "H": H, "arm": arm, "rounds": args.rounds,
                   "calls_per_window": args.calls, "check": check, "ms_median": round(med[arm], 4),
                   "ms_min": round(min(ms[arm]), 4), "ms_max": round(max(ms[arm]), 4),
                   "mrays_s": round(n / med[arm] / 1e3, 1)}
            if arm in against:
                rec["vs"] = against[arm]
                rec["ratio"] = round(med[arm] / med[against[arm]], 4)
            if arm.endswith("_span") and arm.startswith("seg"):
                rec["vs_occluded"] = round(med[arm] / med["occluded"], 4)
            line = json.dumps(rec)
            print(line)
            fh.write(line + "\n")
    for arm, (r, call) in arms:
        r.close()


def sky_pixels(r, desc, dirs, rgb) -> int:
    """Pixels of the depth-1 frame ``rgb`` whose colour is the sky's.  A miss at depth 1 returns
    clamp(skybox texel x envColor) (Scene.cpp:226-231) and a hit a shaded colour, so a pixel counts as sky when its
    colour is that product for its own ray: the texel from the library's skybox known-answer entry, envColor
    summed as Scene.cpp:12,55 sums it (diffuse colour x power, then every light's colour x power), in float32."""
    f32 = np.float32
    texel = r.kat_texels(-1, dirs)
    env = np.array(desc.diffuse[:3], f32) * f32(desc.diffuse[3])
    for (_, _, c, power) in desc.lights:
        env = env + np.array(c, f32) * f32(power)
    sky = np.clip(texel * env[None, :] + f32(0.0), f32(0.0), f32(1.0)).astype(f32)
    return int((rgb.reshape(-1, 3).view(np.uint32) == sky.view(np.uint32)).all(axis=1).sum())


if __name__ == "__main__":
    main()
