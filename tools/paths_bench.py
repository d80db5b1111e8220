#!/usr/bin/env python3
"""Paths against the one-shot ray batch (GPU box): what the state between segments costs and what a wavefront loop over
it gains or loses, by tools/rays_bench.py's method -- ONE process on ONE GPU, the arms interleaved, every window between
two device events, medians over the rounds.

    python tools/paths_bench.py --config c3 [--permuted] [--rounds R] [--calls F] [--out DIR]
    python tools/paths_bench.py --config c5 [--permuted] ...

c3: synth16 3840x2160 depth 8 (BASELINE C3); c5: stress4096 3840x2160 depth 12 (C5).  The rays are cameras.pinhole_rays
of the scene's camera, in frame order or (--permuted) in a fixed random permutation: what incoherent callers hold.

Arms (every one its own renderer on the same scene and stream; a call is the whole image from rays to colours, pre-pass
included):
    batch, batch_again  rfx_trace_rays, raster_width 0; twice, so the pair's difference is the run's own noise band
    one_step            rfx_paths_begin + one rfx_paths_step to the full depth: the one-shot kernel's work plus the
                        state's loads and stores
    per_segment         begin, then a step per segment over the live list (the count read back after every step: the
                        host sizes the next launch by it)
    per_segment_order   the same with rfx_paths_order on the live list before every step but the first
Before anything is timed every arm's colours and ARGB words are hashed against batch's from the same seed.
One JSON line per arm goes to stdout and to DIR/paths_<config>[_permuted].jsonl (default profiles/r19).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reflaxman_amd import _lib, cameras, scenes  # noqa: E402
from reflaxman_amd.render import Renderer, build_scene  # noqa: E402

CONFIGS = {"c3": ("synth16", 3840, 2160, 8), "c5": ("stress4096", 3840, 2160, 12)}
SEED = 1350490027


def sha(t) -> str:
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c3")
    ap.add_argument("--permuted", action="store_true", help="the rays in a fixed random permutation")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=0, help="calls per timed window (0: 20 for c3, 6 for c5)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paths_bench: no GPU (a timing needs one)")
    name, W, H, depth = CONFIGS[args.config]
    calls = args.calls or (20 if args.config == "c3" else 6)
    scene, cam = build_scene(scenes.get_scene(name))
    n = W * H
    host_rays = cameras.pinhole_rays(tuple(cam.eye), cam.view, cam.fov, W, H)
    if args.permuted:
        host_rays = host_rays[np.random.default_rng(12).permutation(n)]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = C.c_void_p(stream.cuda_stream)
    rays = torch.from_numpy(np.ascontiguousarray(host_rays)).cuda()
    del host_rays
    L = _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    f32 = lambda w: torch.zeros((n, w), dtype=torch.float32, device="cuda")
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
    # one set of planes serves every paths arm (the arms run in turn); begin rewrites all but the records, which a step
    # overwrites: every call copies them in first, on the device, as a caller who keeps its rays would
    cur = torch.empty_like(rays)
    mul, colour, rand, state, argb = f32(3), f32(3), f32(3), i32(n), i32(n)
    planes = _lib.PathPlanes(d_rays=cur.data_ptr(), d_mul=mul.data_ptr(), d_colour=colour.data_ptr(),
                             d_rand=rand.data_ptr(), d_state=state.data_ptr(), d_argb=argb.data_ptr())
    lists = [i32(n + 1), i32(n + 1)]  # ping-pong live lists, each followed by its count
    sorted_list = i32(n)
    rgb_b, argb_b = f32(3), i32(n)
    live_log = []

    def renderer():
        r = Renderer(sphere_seed=SEED, jitter_seed=0)
        r.set_stream(stream.cuda_stream)
        r.set_scene(scene)
        return r

    def batch_arm():
        r = renderer()
        return r, lambda: _lib.check(L.rfx_trace_rays(r._h, ptr(rays), n, depth, 0, ptr(rgb_b), ptr(argb_b), None, st),
                                     "rfx_trace_rays")

    def begin(r):
        cur.copy_(rays)
        _lib.check(L.rfx_paths_begin(r._h, C.byref(planes), n, 1, st), "rfx_paths_begin")

    def one_step_arm():
        r = renderer()

        def call():
            begin(r)
            _lib.check(L.rfx_paths_step(r._h, C.byref(planes), n, None, n, depth, None, None, st), "rfx_paths_step")
        return r, call

    def per_segment_arm(order):
        r = renderer()

        def call():
            begin(r)
            index, slots, log = None, n, []
            for k in range(1, depth + 1):
                out = lists[k & 1]
                if order and index is not None:
                    _lib.check(L.rfx_paths_order(r._h, C.byref(planes), n, ptr(index), slots, ptr(sorted_list), st),
                               "rfx_paths_order")
                    index = sorted_list
                _lib.check(L.rfx_paths_step(r._h, C.byref(planes), n, None if index is None else ptr(index), slots, k,
                                            ptr(out), C.c_void_p(out.data_ptr() + 4 * n), st), "rfx_paths_step")
                slots = int(out[n].item())  # (waits for the step)
                log.append(slots)
                if not slots:
                    break
                index = out
            live_log[:] = log
        return r, call

    arms = [("batch", batch_arm()), ("one_step", one_step_arm()), ("per_segment", per_segment_arm(False)),
            ("per_segment_order", per_segment_arm(True)), ("batch_again", batch_arm())]

    # parity: every arm's first call from the seed against batch's
    ok, want, live = {}, None, {}
    for arm, (r, call) in arms:
        for t in (rgb_b, argb_b, colour, argb):
            t.zero_()
        call()
        stream.synchronize()
        r.synchronize()
        got = (sha(rgb_b), sha(argb_b)) if arm.startswith("batch") else (sha(colour), sha(argb))
        if want is None:
            want = got
        ok[arm] = got == want
        if not ok[arm]:
            raise SystemExit(f"{arm}: the output differs from batch's")
        if arm.startswith("per_segment"):
            live[arm] = list(live_log)
    for arm, (r, call) in arms:  # warm-up: every later call continues the random stream, as the timed ones do
        for _ in range(2):
            call()
    stream.synchronize()
    ms = {arm: [] for arm, _ in arms}
    for _ in range(args.rounds):
        for arm, (r, call) in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                call()
            e1.record(stream)
            e1.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / calls)
    base = statistics.median(ms["batch"])
    os.makedirs(args.out, exist_ok=True)
    tag = args.config + ("_permuted" if args.permuted else "")
    with open(os.path.join(args.out, f"paths_{tag}.jsonl"), "w") as f:
        for arm, (r, call) in arms:
            med = statistics.median(ms[arm])
            rec = {"config": args.config, "scene": name, "W": W, "H": H, "depth": depth, "permuted": args.permuted,
                   "arm": arm, "rounds": args.rounds, "calls_per_window": calls, "sha_ok": ok[arm],
                   "ms_median": round(med, 4), "ms_min": round(min(ms[arm]), 4), "ms_max": round(max(ms[arm]), 4),
                   "mrays_s": round(n / med / 1e3, 1), "vs_batch": round(med / base, 4)}
            if arm in live:
                rec["live_after_segment"] = live[arm]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            r.close()


if __name__ == "__main__":
    main()
