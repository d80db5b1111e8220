"""Every entry of the batch launch tables is reached and writes (rfx_batch_launch.h: the trace table's 18 render and 8
counting instantiations, the query table's six, each in its linear / raster kernel and in its ordered one).

One small scene per culling cfg the launch rule can produce -- one light, several, more than 32; small or not; with or
without a plane; the non-small ones also with the triangle tree -- and 65 rays (a full wave and a lane) through every
form of every call into buffers full of a sentinel.  A table entry that launched nothing would leave the sentinel; an
entry that launched the wrong instantiation would miss the CPU references, which every form must equal bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from hits_helpers import PLANES, any_hit, compose, same_bits
from rays_helpers import SEED, incoherent_rays, oracle_trace
from reflaxman_amd import _lib, scenes

pytestmark = pytest.mark.gpu

N, DEPTH, RASTER = 65, 4, 12
SENT, SENT8 = 0x5A5A5A5A, 0x5A
# (lights, small, plane, triangle tree)
CASES = [(li, sm, pl, False) for li in (1, 3, 40) for sm in (True, False) for pl in (False, True)] + \
        [(li, False, pl, True) for li in (1, 3, 40) for pl in (False, True)]
_REF = {}


def describe(lights, small, plane, mesh):
    """The default scene's pieces (its sun, its 8 spheres, its checker ground pair), then what the case adds: lights on
    a ring above the scene (lights_scene's), 25 generated spheres (33 in all: not small), a 48-triangle height field,
    a floor plane.  Spheres, then triangles, then planes: the order the kernels visit them."""
    base = scenes.default_scene()
    d = scenes.SceneDesc(f"cfg_l{lights}_{'small' if small else 'large'}{'_plane' if plane else ''}{'_mesh' if mesh else ''}",
                         base.diffuse, base.camera)
    d.lights.append(base.lights[0])
    g = scenes.Lcg(4040 + lights)
    for k in range(lights - 1):
        ang = 2.0 * np.pi * k / (lights - 1)
        d.add_light((6.0 * np.cos(ang) + g.uniform(-1, 1), g.uniform(4.0, 9.0), 5.0 * np.sin(ang) + g.uniform(-1, 1)),
                    g.uniform(0.2, 1.5), (g.uniform(0.4, 1), g.uniform(0.4, 1), g.uniform(0.4, 1)), 0.8 / lights)
    d.objects += [ob for ob in base.objects if ob[0] == "sphere"]
    if not small:
        g = scenes.Lcg(20261015)
        for _ in range(25):
            rad = g.uniform(0.1, 0.6)
            c = (g.uniform(-12.0, 12.0), rad, g.uniform(-9.0, 9.0))
            d.add_sphere(c, rad, scenes.DIELECTRIC if g.next_u32() >> 31 else scenes.METAL,
                         (g.uniform(0, 1), g.uniform(0, 1), g.uniform(0, 1)), g.uniform(0, 1))
    ti = d.add_texture(scenes.Texture("himiya", None))
    for ob in base.objects:
        if ob[0] == "triangle":
            d.objects.append(ob)
    for (oi, _, uv) in base.settex:
        d.set_texture(len(d.objects) - 2 + (oi - base.settex[0][0]), ti, uv)
    if mesh:
        g = scenes.Lcg(777)
        nx, nz = 6, 4
        verts = [(-6.0 + 2.0 * i, g.uniform(0.05, 0.4), -4.0 + 2.0 * j) for i in range(nx + 1) for j in range(nz + 1)]
        at = lambda i, j: i * (nz + 1) + j
        idx = []
        for i in range(nx):
            for j in range(nz):
                idx += [(at(i, j), at(i, j + 1), at(i + 1, j)), (at(i, j + 1), at(i + 1, j + 1), at(i + 1, j))]
        d.add_mesh(verts, idx, scenes.METAL, (0.7, 0.8, 0.6), 0.4)
    if plane:
        d.add_plane((0.0, -0.05, 0.0), (0.0, 2.0, 0.0), scenes.DIELECTRIC, (0.8, 0.85, 0.9), 0.6)
    return d


def rays():
    """rays_helpers' fixed rays of the default scene, whose box these scenes share: no zero components"""
    return incoherent_rays("default")[:N]


def reference(case):
    """(description, oracle colours, oracle counters, composed closest-hit planes, composed table), once per case"""
    if case not in _REF:
        d = describe(*case)
        cnt = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
        rgb, _ = oracle_trace(d, rays(), DEPTH, SEED, cnt)
        assert np.isfinite(rgb).all(), case
        planes, tab = compose(d, rays(), key=("batch_cfgs", case))
        for a in (rgb, cnt):
            a.setflags(write=False)
        _REF[case] = (d, rgb, cnt, planes, tab)
    return _REF[case]


def dev(a):
    import torch
    a = np.array(a)  # (a copy: the shared references are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def filled(words, byte=False):
    import torch
    return torch.full((words,), SENT8 if byte else SENT, dtype=torch.uint8 if byte else torch.int32, device="cuda")


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def run(r, call):
    """One C entry point on the renderer's own stream, fenced on both sides (it is not ordered with torch's)"""
    import torch
    torch.cuda.synchronize()
    _lib.check(call())
    r.synchronize()


FORMS = ("linear", "raster", "ordered")


def trace(r, L, d_rays, d_order, form, counters=None):
    """(colours (N, 3) float32, ARGB words (N,) uint32) of one form of rfx_trace_rays from SEED, out of sentinel-filled
    buffers in which no sentinel may remain"""
    rgb, argb = filled(3 * N), filled(N)
    r.set_rng(SEED, 77)
    if form == "ordered":
        run(r, lambda: L.rfx_trace_rays_ordered(r._h, ptr(d_rays), ptr(d_order), N, DEPTH, ptr(rgb), ptr(argb), None))
    else:
        run(r, lambda: L.rfx_trace_rays(r._h, ptr(d_rays), N, DEPTH, RASTER if form == "raster" else 0, ptr(rgb),
                                        ptr(argb), ptr(counters), None))
    rgb, argb = rgb.cpu().numpy(), argb.cpu().numpy().view(np.uint32)
    assert not (rgb == SENT).any() and not (argb == SENT).any(), (form, "a sentinel remains")
    return rgb.view(np.float32).reshape(N, 3), argb


def query(r, L, d_rays, d_order, form):
    buf = {k: filled(N * (1 if k in ("object", "distance") else 3)) for k in PLANES}
    hp = _lib.HitPlanes()
    for k in PLANES:
        setattr(hp, k, buf[k].data_ptr())
    if form == "ordered":
        run(r, lambda: L.rfx_query_hits_ordered(r._h, ptr(d_rays), ptr(d_order), N, C.byref(hp), None))
    else:
        run(r, lambda: L.rfx_query_hits(r._h, ptr(d_rays), N, RASTER if form == "raster" else 0, C.byref(hp), None))
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    for k in PLANES:
        assert not (out[k] == SENT).any(), (form, k, "a sentinel remains")
    return out


def shadow(r, L, d_rays, d_order, d_skip, form):
    occ = filled(N, byte=True)
    if form == "ordered":
        run(r, lambda: L.rfx_query_occluded_ordered(r._h, ptr(d_rays), ptr(d_skip), ptr(d_order), N, ptr(occ), None))
    else:
        run(r, lambda: L.rfx_query_occluded(r._h, ptr(d_rays), ptr(d_skip), N, RASTER if form == "raster" else 0,
                                            ptr(occ), None))
    occ = occ.cpu().numpy()
    assert not (occ == SENT8).any(), (form, "a sentinel remains")
    return occ


@pytest.mark.parametrize("case", CASES, ids=lambda c: "l%d-%s%s%s" % (c[0], "small" if c[1] else "large",
                                                                     "-plane" if c[2] else "", "-tree" if c[3] else ""))
def test_every_form_of_every_call_writes_the_reference(case):
    import torch
    from reflaxman_amd.render import Renderer, build_scene
    lights, small, plane, tree = case
    d, want, ocnt, planes, tab = reference(case)
    assert (d.n_spheres <= 32 and d.n_triangles <= 32) == small and len(d.lights) == lights
    s, cam = build_scene(d)
    r = Renderer(sphere_seed=SEED, jitter_seed=77)
    r.set_tri_accel(1 if tree else 0)
    r.set_scene(s)
    assert (r.accel_info().tri_nodes > 0) == tree
    L = _lib.load()
    d_rays, d_order = dev(rays()), dev(np.arange(N, dtype=np.uint32)[::-1])
    words = orc.argb_of(want)
    for form in FORMS:
        rgb, argb = trace(r, L, d_rays, d_order, form)
        bad = same_bits(rgb, want)
        assert bad.size == 0, (case, form, bad[:8].tolist(), rgb[bad[:2]].tolist(), want[bad[:2]].tolist())
        assert np.array_equal(argb, words), (case, form)
    # the counting kernels: the render kernels' colours, the oracle's counts.  More than 32 spheres: the kernel visits
    # them in Morton order, so the shadow any-hit, which stops at the first occluder, runs another number of tests than
    # the oracle's insertion order (test_gpu_parity.py test_event_counters_match_oracle); every other count is equal.
    for form in ("linear", "raster"):
        cnt = torch.zeros(_lib.RFX_NCOUNTERS, dtype=torch.int64, device="cuda")
        rgb, argb = trace(r, L, d_rays, None, form, counters=cnt)
        assert same_bits(rgb, want).size == 0 and np.array_equal(argb, words), (case, form, "stats")
        gc = cnt.cpu().numpy().view(np.uint64)
        off = {k: (int(a), int(b)) for k, a, b in zip(orc.COUNTER_NAMES, gc, ocnt)
               if a != b and not (k.startswith("sh_") and d.n_spheres > 32)}
        assert not off, (case, form, off)
    d_skip = dev(planes["object"])
    for form in FORMS:
        got = query(r, L, d_rays, d_order, form)
        for k in PLANES:
            g = got[k].view(planes[k].dtype).reshape(planes[k].shape)
            bad = same_bits(g, planes[k])
            assert bad.size == 0, (case, form, k, bad[:8].tolist(), g[bad[:2]].tolist(), planes[k][bad[:2]].tolist())
        assert np.array_equal(shadow(r, L, d_rays, d_order, None, form), any_hit(tab)), (case, form)
        assert np.array_equal(shadow(r, L, d_rays, d_order, d_skip, form), any_hit(tab, planes["object"])), (case, form)
    r.close()
