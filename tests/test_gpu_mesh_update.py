"""Moving meshes on the device (rfx.h "Moving meshes", rfx_renderer_update_triangles): after an update every launch is
the one a renderer gives whose set_scene got the scene built at the new vertices -- the records and the refitted tree
bit for bit against the host mirror, frames of every mode against the oracle of the moved scene, the batch calls against
a fresh renderer's."""
import ctypes as C

import numpy as np
import pytest

from mesh_update import F, SEED, case1_vertices, moved_desc, pooled, tri_vertices, wave
from reflaxman_amd import _lib, scenes

pytestmark = pytest.mark.gpu

_DESC, _BUILT, _REF = {}, {}, {}


def desc_of(key):
    if key not in _DESC:
        _DESC[key] = {"mesh": lambda: scenes.mesh_scene(16, 12), "degenerate": scenes.degenerate_soup_scene,
                      "soup33": lambda: scenes.soup_scene(31), "soup300": lambda: scenes.soup_scene(300),
                      "soup298s8": lambda: scenes.soup_scene(298, n_spheres=8),
                      "soup38s8": lambda: scenes.soup_scene(38, n_spheres=8),
                      "soup1500s300": lambda: scenes.soup_scene(1500, n_spheres=300)}[key]()
    return _DESC[key]


def built(key):
    """(Scene, Camera) of a case as its description has it, built once (never edited: a test that edits builds its own)"""
    if key not in _BUILT:
        from reflaxman_amd.render import build_scene
        _BUILT[key] = build_scene(desc_of(key))
    return _BUILT[key]


def oracle_frame(tag, desc, W, H, depth, ss=1, seed=SEED):
    """The oracle's frame of `desc`, computed once per tag, shared, read-only"""
    k = (tag, W, H, depth, ss, seed)
    if k not in _REF:
        import oracle as orc
        o = orc.OracleRender(desc, seed, 0)
        o.set_image_size(W, H)
        o.render(depth, ss)
        o.image.setflags(write=False)
        _REF[k] = (o.image, o.sphere_seed.value)
    return _REF[k][0]


def renderer(scene, mode, seed=SEED, **knobs):
    from reflaxman_amd.render import Renderer
    rr = Renderer(sphere_seed=seed, jitter_seed=0)
    rr.set_tri_accel(mode)
    for name, v in knobs.items():
        getattr(rr, "set_" + name)(v)
    rr.set_scene(scene)
    return rr


def frame(rr, cam, W, H, depth, ss=1):
    from reflaxman_amd.render import make_frame
    img = np.zeros((H, W, 3), F)
    f = make_frame(cam, W, H, depth, ss)
    _lib.check(_lib.load().rfx_render_frame_host(rr._h, C.byref(f), _lib.fptr(img), None, None), "render_frame_host")
    return img


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_nodes(scene, V):
    boxes, mt = scene.tri_bvh_refit(V, widen=True)
    return boxes, scene.tri_bvh_dump()["children"], mt


def same_nodes(got, want):
    return all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def make_ill(V, tris):
    """the triangles `tris` of V turned into four slivers (cond >= 300), a zero-area triangle and a NaN vertex"""
    V = V.copy()
    for k, t in enumerate(tris[:4]):
        a, b = V[t, 0].astype(np.float64), V[t, 1].astype(np.float64)
        V[t, 2] = (a + 0.3 * (b - a) + 1e-4 * np.linalg.norm(b - a) * np.roll(np.eye(3)[k % 3], 1)).astype(F)
    if len(tris) > 4:
        V[tris[4], 2] = V[tris[4], 1]
    if len(tris) > 5:
        V[tris[5], 0, 1] = np.nan
    return V


def rays_at_the_scene(n=4096, seed=5):
    rng = np.random.default_rng(seed)
    o = rng.uniform((-14, 0.3, -12), (14, 9, 10), (n, 3))
    q = rng.uniform((-12, 0.0, -9), (12, 5, 9), (n, 3))
    return np.concatenate([o, (q - o) * rng.uniform(0.2, 3.0, (n, 1))], axis=1).astype(F)


# ------------------------------------------------------------------------------------------------ records and nodes
def test_records_after_a_whole_scene_update():
    """mesh_update.case1_vertices (soup, slivers, zero-area, coincident, huge, subnormal, NaN and infinite) over a 300-triangle
    scene with 8 spheres: the device's words are the edited host scene's, and the tree's copy follows"""
    from reflaxman_amd.render import build_scene
    s, _ = build_scene(desc_of("soup298s8"))
    rr = renderer(s, 1)
    assert rr.accel_info().tri_nodes > 0
    assert rr.tri_records().tobytes() == s.tri_records().tobytes()
    V = case1_vertices()
    rr.update_triangles(0, dev(V))
    s.setTriangleVertices(0, V)
    got, want = rr.tri_records(), s.tri_records()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.tobytes() == want.tobytes(), (bad[:8].tolist(), [np.flatnonzero(got[b] != want[b]).tolist() for b in bad[:4]])
    rr.close()


@pytest.mark.parametrize("key", ["mesh", "degenerate", "soup33"])
def test_nodes_follow_the_host_refit_and_come_back(key):
    """A -> B -> C -> A: after every update the device's nodes are the host refit's (the device copy, widen = 1), bit
    for bit, and back at A both the nodes and the records are those set_scene(A) left -- no drift"""
    s, _ = built(key)
    A = tri_vertices(desc_of(key))
    rr = renderer(s, 1)
    nodes_a, rec_a = rr.tri_bvh_nodes(), rr.tri_records()
    assert same_nodes(nodes_a, host_nodes(s, A))
    rng = np.random.default_rng(3)
    B = wave(A, amp=0.3)
    Cv = (wave(A, amp=1.5, phase=1.0) + rng.uniform(-2.0, 2.0, A.shape)).astype(F)
    for name, V in (("B", B), ("C", Cv)):
        rr.update_triangles(0, dev(V))
        got, want = rr.tri_bvh_nodes(), host_nodes(s, V)
        assert same_nodes(got, want), (key, name, int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum()),
                                       int((got[2].view(np.uint32) != want[2].view(np.uint32)).sum()))
        assert not same_nodes(got, nodes_a)
    rr.update_triangles(0, A)  # the host form
    assert same_nodes(rr.tri_bvh_nodes(), nodes_a)
    assert rr.tri_records().tobytes() == rec_a.tobytes()
    rr.close()


# ------------------------------------------------------------------------------------------------ frames
FRAMES = [(64, 36, 1, {}), (64, 36, 1, {"regroup": 0}), (64, 36, 1, {"regroup": 1}), (64, 36, 1, {"launch_traces": 500}),
          (32, 18, 4, {}), (16, 9, 16, {}), (48, 27, -3, {})]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("W,H,ss,knobs", FRAMES, ids=str)
def test_mesh_frames_after_a_wave(mode, W, H, ss, knobs):
    """mesh16x12 with a height wave on every vertex (the indexed form, torch tensors): the oracle's frame of the moved
    scene under every tri-accel mode, schedule knob and sampling mode"""
    s, cam = built("mesh")
    V = wave(tri_vertices(desc_of("mesh")))
    ref = oracle_frame("mesh_wave", moved_desc(desc_of("mesh"), V), W, H, 6, ss)
    rr = renderer(s, mode, **knobs)
    pool, idx = pooled(V)
    assert len(pool) < V.shape[0] * 3 // 2
    rr.update_triangles(0, dev(pool), dev(idx.view(np.int32)))
    img = frame(rr, cam, W, H, 6, ss)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    assert (rr.accel_info().tri_nodes > 0) == (mode > 0)
    rr.close()


def test_event_counters_after_a_wave():
    """the stats kernel's event counters on the updated scene are the oracle's on the moved scene"""
    import oracle as orc
    from reflaxman_amd.render import make_frame
    s, cam = built("mesh")
    desc = desc_of("mesh")
    V = wave(tri_vertices(desc))
    W, H, depth = 48, 27, 6
    o = orc.OracleRender(moved_desc(desc, V), 4242, 0)
    o.set_image_size(W, H)
    oc = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
    o.render(depth, 1, counters=oc)
    rr = renderer(s, 1, seed=4242)
    rr.update_triangles(0, dev(V))
    img, gc = np.zeros((H, W, 3), F), np.zeros(len(orc.COUNTER_NAMES), np.uint64)
    f = make_frame(cam, W, H, depth, 1)
    _lib.check(_lib.load().rfx_render_frame_host(rr._h, C.byref(f), _lib.fptr(img), None, _lib.u64ptr(gc)))
    assert img.tobytes() == o.image.tobytes()
    bad = {k: (int(a), int(b)) for k, a, b in zip(orc.COUNTER_NAMES, gc, oc) if a != b}
    assert not bad, bad
    rr.close()


def test_update_between_two_frames_on_one_stream():
    """frame, update, frame enqueued on one stream with no host sync between: the first is the old scene's, the second
    the moved scene's from the stream state the first left; the update leaves both random streams alone"""
    import oracle as orc
    import torch
    from reflaxman_amd.render import make_frame
    s, cam = built("mesh")
    desc = desc_of("mesh")
    V = wave(tri_vertices(desc), amp=0.35, phase=2.0)
    W, H, depth = 64, 36, 6
    o1 = orc.OracleRender(desc, SEED, 0)
    o1.set_image_size(W, H)
    o1.render(depth, 1)
    seed1 = o1.sphere_seed.value
    o2 = orc.OracleRender(moved_desc(desc, V), seed1, 0)
    o2.set_image_size(W, H)
    o2.render(depth, 1)
    rr = renderer(s, 1)
    f = make_frame(cam, W, H, depth, 1)
    pool, idx = pooled(V)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_pool, d_idx = dev(pool), dev(idx.view(np.int32))
        img = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        st.synchronize()  # (the inputs are in place; nothing below waits on the host)
        rr.render_frame(f, img[0].data_ptr(), stream=st.cuda_stream)
        rr.update_triangles(0, d_pool, d_idx)
        rr.render_frame(f, img[1].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert img[0].cpu().numpy().tobytes() == o1.image.tobytes()
    assert img[1].cpu().numpy().tobytes() == o2.image.tobytes()
    assert rr.get_rng()[0] == o2.sphere_seed.value
    # the streams before and after an update on its own
    rr.set_rng(seed1, 77)
    before = rr.get_rng()
    rr.update_triangles(0, d_pool, d_idx)
    assert rr.get_rng() == before == (seed1, 77)
    rr.close()


PARTIAL = ["one", "across_leaves", "last", "dead_index"]


@pytest.mark.parametrize("what", PARTIAL)
def test_partial_updates(what):
    """count = 1, a range crossing leaf boundaries, the last triangle, an indexed update naming one vertex that does not
    exist: the oracle's frame, the untouched triangles' words unchanged, the whole tree the host refit's"""
    s, cam = built("mesh")
    desc = desc_of("mesh")
    A = tri_vertices(desc)
    n = len(A)
    moved = (wave(A, amp=0.6, phase=0.5) + F(0.05)).astype(F)
    rr = renderer(s, 1)
    before = rr.tri_records()
    first, count = {"one": (5, 1), "across_leaves": (10, 23), "last": (n - 1, 1), "dead_index": (40, 9)}[what]
    V = A.copy()
    V[first:first + count] = moved[first:first + count]
    if what == "dead_index":
        pool, idx = pooled(moved[first:first + count])
        idx[4, 1] = len(pool)  # triangle first + 4 keeps its vertices
        V[first + 4] = A[first + 4]
        rr.update_triangles(first, dev(pool), dev(idx.view(np.int32)))
    elif what == "last":
        rr.update_triangles(first, moved[first:first + count])  # the host form
    else:
        rr.update_triangles(first, dev(moved[first:first + count]))
    after = rr.tri_records()
    changed = np.zeros(n, bool)
    changed[first:first + count] = True
    if what == "dead_index":
        changed[first + 4] = False
    assert after[~changed].tobytes() == before[~changed].tobytes()
    assert (after[changed] != before[changed]).any(axis=1).all()
    assert same_nodes(rr.tri_bvh_nodes(), host_nodes(s, V))
    W, H = 64, 36
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("mesh_" + what, moved_desc(desc, V), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


# ------------------------------------------------------------------------------------------------ class changes
_CLASS = {}


def class_change():
    """soup300 with six in-tree triangles turned ill-conditioned: (moved vertices, the edited Scene, its description)"""
    if not _CLASS:
        from reflaxman_amd.render import build_scene
        desc = desc_of("soup300")
        s, _ = built("soup300")
        ids = s.tri_bvh_dump()["leaf_ids"]
        six = [int(t) for t in ids[[0, 3, 17, 30, 41, 55], 0]]
        V = make_ill(tri_vertices(desc), six)
        edited, _ = build_scene(moved_desc(desc, V))
        _CLASS.update(V=V, six=six, edited=edited, desc=moved_desc(desc, V))
    return _CLASS


@pytest.mark.parametrize("mode", [1, 2])
def test_class_change_frames(mode):
    """triangles of the tree that turn into slivers, a zero-area triangle and a NaN vertex are still tested by every
    ray: the oracle's frame"""
    c = class_change()
    s, cam = built("soup300")
    rr = renderer(s, mode)
    rr.update_triangles(0, dev(c["V"]))
    rec = rr.tri_records()
    assert (rec[c["six"], 28] == 0).all() and (rec[c["six"], 18] == F(np.inf).view(np.uint32)).all()
    boxes = rr.tri_bvh_nodes()[0]
    assert np.isnan(boxes[0]).any()  # a child of the root holds one of the six
    W, H = 48, 27
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("soup300_ill", c["desc"], W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


def test_class_change_queries_equal_a_fresh_renderer():
    """query_hits (all planes), occluded and the span form on 4,096 rays: a fresh renderer's after set_scene of the
    edited scene"""
    c = class_change()
    s, _ = built("soup300")
    rays = rays_at_the_scene()
    rr, fresh = renderer(s, 1), renderer(c["edited"], 1)
    rr.update_triangles(0, dev(c["V"]))
    assert fresh.accel_info().tri_residual == rr.accel_info().tri_residual + 6  # a fresh build moves them out of the tree
    a, b = rr.query_hits(rays), fresh.query_hits(rays)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["object"] >= 0).sum() > 1000
    assert rr.occluded(rays).tobytes() == fresh.occluded(rays).tobytes()
    lo = np.where(a["object"] < 0, F(np.inf), a["distance"])
    a2, b2 = rr.query_hits(rays, lo=lo, after=a["object"]), fresh.query_hits(rays, lo=lo, after=a["object"])
    for k in a2:
        assert a2[k].tobytes() == b2[k].tobytes(), k
    assert (a2["object"] >= 0).sum() > 300
    rr.close()
    fresh.close()


def test_no_tree_bound_follows_the_class():
    """40 triangles and 8 spheres at the default tri-accel (the chunk loops cull by `bound`), one triangle made
    ill-conditioned and the rest moved: the oracle's frame"""
    s, cam = built("soup38s8")
    desc = desc_of("soup38s8")
    V = make_ill(wave(tri_vertices(desc), amp=0.3), [7])
    rr = renderer(s, -1)
    assert rr.accel_info().tri_nodes == 0 and rr.tri_bvh_nodes() is None
    rr.update_triangles(0, dev(V))
    assert rr.tri_records()[7, 28] == 0
    W, H = 48, 27
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("soup38_ill", moved_desc(desc, V), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


def test_both_trees_parked_frame():
    """1500 soup triangles under 300 spheres: the sphere tree stays, the triangle tree is refitted from its reference
    point; the parked frame with the LDS-staged bounce kernel is the oracle's"""
    s, cam = built("soup1500s300")
    desc = desc_of("soup1500s300")
    V = wave(tri_vertices(desc), amp=0.4)
    rr = renderer(s, 1)
    rr.update_triangles(0, dev(V))
    assert same_nodes(rr.tri_bvh_nodes(), host_nodes(s, V))
    W, H = 48, 27
    img = frame(rr, cam, W, H, 6)
    assert rr.bounce_form() == 2 and rr.accel_info().sph_nodes > 0
    ref = oracle_frame("soup1500_wave", moved_desc(desc, V), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


def test_batch_calls_equal_a_fresh_renderer():
    """trace_rays, its coherent order (the updated renderer keeps the old key box: a schedule input) and one paths step
    on 4,096 rays, from one stream state"""
    from reflaxman_amd.render import build_scene
    desc = desc_of("mesh")
    s, _ = built("mesh")
    V = wave(tri_vertices(desc), amp=0.5)
    edited, _ = build_scene(moved_desc(desc, V))
    rays = rays_at_the_scene(seed=9)
    rr, fresh = renderer(s, 1), renderer(edited, 1)
    rr.update_triangles(0, dev(V))
    assert not np.array_equal(rr.order_box()[0], fresh.order_box()[0])  # the wave moved the box's floor
    for kw in ({}, {"order": "coherent"}):
        rr.set_rng(SEED, 0)
        fresh.set_rng(SEED, 0)
        a, b = rr.trace_rays(rays, 6, **kw), fresh.trace_rays(rays, 6, **kw)
        assert a.tobytes() == b.tobytes(), kw
        assert rr.get_rng() == fresh.get_rng()
    rr.set_rng(SEED, 0)
    fresh.set_rng(SEED, 0)
    pa, pb = rr.paths(rays), fresh.paths(rays)
    pa.step(1)
    pb.step(1)
    for k in ("rays", "mul", "colour", "state"):
        assert getattr(pa, k).tobytes() == getattr(pb, k).tobytes(), k
    pa.close()
    pb.close()
    rr.close()
    fresh.close()


def test_two_member_group_after_host_updates():
    """a device group of two members on device 0, the host-form update on both members' renderers: the group's frame
    is the single renderer's and the oracle's"""
    import torch
    from reflaxman_amd.render import make_frame
    L = _lib.load()
    s, cam = built("mesh")
    desc = desc_of("mesh")
    V = np.ascontiguousarray(wave(tri_vertices(desc)))
    W, H = 64, 36
    g = C.c_void_p()
    _lib.check(L.rfx_group_create(C.byref(g), (C.c_int * 2)(0, 0), 2), "group_create")
    for m in range(2):
        _lib.check(L.rfx_renderer_set_tri_accel(C.c_void_p(L.rfx_group_renderer(g, m)), 1))
    _lib.check(L.rfx_group_set_scene(g, s._h), "group_set_scene")
    for m in range(2):
        _lib.check(L.rfx_renderer_update_triangles_host(C.c_void_p(L.rfx_group_renderer(g, m)), 0, len(V), _lib.fptr(V),
                                                        3 * len(V), None), "update_triangles_host")
    _lib.check(L.rfx_renderer_set_rng(C.c_void_p(L.rfx_group_renderer(g, 0)), SEED, 0))
    one = renderer(s, 1)
    one.update_triangles(0, V)
    f = make_frame(cam, W, H, 6, 1)
    bufs = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    _lib.check(L.rfx_group_render_frame(g, C.byref(f), C.c_void_p(bufs[0].data_ptr()), None, None))
    one.render_frame(f, bufs[1].data_ptr())
    one.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])
    ref = oracle_frame("mesh_wave", moved_desc(desc, V), W, H, 6)
    assert bufs[0].cpu().numpy().tobytes() == ref.tobytes()
    L.rfx_group_destroy(g)
    one.close()


def test_errors():
    from reflaxman_amd.render import Renderer, build_scene
    L = _lib.load()
    s, _ = built("mesh")
    n = desc_of("mesh").n_triangles
    v = np.zeros((4, 9), F)
    zeros = np.zeros(12, np.uint32)
    p, i = _lib.fptr(v), _lib.u32ptr(zeros)
    rr = Renderer(sphere_seed=SEED)
    assert L.rfx_renderer_update_triangles_host(rr._h, 0, 1, p, 3, None) == -3  # no scene uploaded
    rr.set_scene(s)
    ARG, STATE = -1, -3
    assert L.rfx_renderer_update_triangles_host(None, 0, 1, p, 3, None) == ARG
    assert L.rfx_renderer_update_triangles_host(rr._h, 0, 1, None, 3, None) == ARG
    assert L.rfx_renderer_update_triangles_host(rr._h, 0, 0, p, 0, None) == ARG
    assert L.rfx_renderer_update_triangles_host(rr._h, n - 3, 4, p, 12, None) == ARG
    assert L.rfx_renderer_update_triangles_host(rr._h, 0, 4, p, 11, None) == ARG
    assert L.rfx_renderer_update_triangles(rr._h, 0, 4, None, 12, None, None) == ARG
    assert L.rfx_renderer_update_triangles(rr._h, n, 1, C.c_void_p(16), 3, None, None) == ARG
    assert L.rfx_renderer_update_triangles_host(rr._h, 0, 4, p, 11, i) == 0  # with indices any pool size will do
    assert L.rfx_renderer_update_triangles_host(rr._h, n - 4, 4, p, 12, None) == 0
    small, _ = build_scene(scenes.default_scene())
    rr.set_scene(small)
    assert L.rfx_renderer_update_triangles_host(rr._h, 0, 1, p, 3, None) == STATE
    assert b"rfx_renderer_set_scene" in L.rfx_last_error()
    with pytest.raises(_lib.RfxError):
        rr.update_triangles(0, v[:1])
    rr.close()
