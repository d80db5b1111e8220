"""Shared by the paths tests (test_paths_host.py, test_gpu_paths.py): the per-depth oracle of the fixed test rays, the
state planes as sentinel-filled device tensors, and the three C calls on them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from rays_helpers import SEED, incoherent_rays, oracle_trace, scene
from reflaxman_amd import _lib

SENT = 0x5A5A5A5A
WORDS = {"rays": 6, "mul": 3, "colour": 3, "rand": 3, "state": 1, "argb": 1}
DTYPE = {"rays": np.float32, "mul": np.float32, "colour": np.float32, "rand": np.float32, "state": np.int32,
         "argb": np.uint32}
_DEPTHS = {}


def oracle_depths(name, depths=range(1, 9), desc=None, rays=None):
    """{k: colours of Scene::trace(.., k) on incoherent_rays(name) from SEED} -- every Scene::trace takes one draw
    whatever its depth, so ray i meets the same randDir at every k.  Computed once per (name, k)."""
    out = {}
    for k in depths:
        if (name, k) not in _DEPTHS:
            rgb, _ = oracle_trace(desc if desc is not None else scene(name),
                                  rays if rays is not None else incoherent_rays(name), k, SEED)
            rgb.setflags(write=False)
            _DEPTHS[(name, k)] = rgb
        out[k] = _DEPTHS[(name, k)]
    return out


def dev(a):
    import torch
    a = np.array(a)  # (a copy: the shared references are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def run(r, call):
    """One C entry point on the renderer's own stream, fenced on both sides (it is not ordered with torch's)."""
    import torch
    torch.cuda.synchronize()
    rc = call()
    r.synchronize()
    return rc


class State:
    """The planes of len(rays) paths and of `extra` more after them, every word a sentinel but the rays' records (the
    extra paths take real records too: were a dead lane to run, its words would change)."""

    def __init__(self, rays, extra_rays=None, argb=True):
        import torch
        self.n = len(rays)
        self.m = self.n + (0 if extra_rays is None else len(extra_rays))
        self.t = {k: torch.full((self.m * w,), SENT, dtype=torch.int32, device="cuda") for k, w in WORDS.items()}
        all_rays = np.asarray(rays, np.float32) if extra_rays is None else np.concatenate([rays, extra_rays])
        self.t["rays"].copy_(dev(np.ascontiguousarray(all_rays, np.float32).view(np.int32).reshape(-1)))
        self.planes = _lib.PathPlanes(**{"d_" + k: v.data_ptr() for k, v in self.t.items() if k != "argb" or argb})

    def words(self, name):
        """All m paths' words of a plane, (m, w) int32."""
        return self.t[name].cpu().numpy().reshape(self.m, WORDS[name])

    def get(self, name):
        """The n paths' plane in its own type: (n, w), or (n,) for state and argb."""
        a = np.ascontiguousarray(self.words(name)[:self.n]).view(DTYPE[name])
        return a.reshape(self.n) if WORDS[name] == 1 else a

    def snapshot(self):
        return {k: self.words(k).copy() for k in WORDS}


def begin(r, st, draw=1, n=None):
    L = _lib.load()
    return run(r, lambda: L.rfx_paths_begin(r._h, C.byref(st.planes), st.n if n is None else n, draw, None))


def step(r, st, upto, index=None, slots=None, live=False, n=None):
    """rfx_paths_step; live: returns (rc, the live list as written -- uint32, count entries -- , the words after it)."""
    import torch
    L = _lib.load()
    d_index = None if index is None else dev(np.asarray(index, np.uint32))
    slots = (st.n if index is None else len(index)) if slots is None else slots
    d_live = torch.full((slots + 64,), SENT, dtype=torch.int32, device="cuda") if live else None
    d_count = torch.full((1,), SENT, dtype=torch.int32, device="cuda") if live else None
    rc = run(r, lambda: L.rfx_paths_step(r._h, C.byref(st.planes), st.n if n is None else n, ptr(d_index), slots,
                                         upto, ptr(d_live), ptr(d_count), None))
    if not live:
        return rc
    count = int(d_count.cpu().numpy().view(np.uint32)[0])
    words = d_live.cpu().numpy().view(np.uint32)
    return rc, words[:count].copy(), words[count:]


def order(r, st, index=None, slots=None, n=None):
    """rfx_paths_order: (rc, the order's `slots` words, the 64 words after them)."""
    import torch
    L = _lib.load()
    d_index = None if index is None else dev(np.asarray(index, np.uint32))
    slots = (st.n if index is None else len(index)) if slots is None else slots
    d_order = torch.full((slots + 64,), SENT, dtype=torch.int32, device="cuda")
    rc = run(r, lambda: L.rfx_paths_order(r._h, C.byref(st.planes), st.n if n is None else n, ptr(d_index), slots,
                                          ptr(d_order), None))
    words = d_order.cpu().numpy().view(np.uint32)
    return rc, words[:slots].copy(), words[slots:]
