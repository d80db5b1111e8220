"""Moving spheres on the device (rfx.h "Moving spheres", rfx_renderer_update_spheres): after an update every launch is
the one a renderer gives whose set_scene got the scene built at the new spheres -- the records, the chunk bounds and the
refitted pair tree bit for bit against the host mirror, frames of every mode against the oracle of the moved scene, the
batch calls against a fresh renderer's."""
import ctypes as C

import numpy as np
import pytest

from mesh_update import tri_vertices, wave
from mesh_update import moved_desc as moved_tris
from reflaxman_amd import _lib, scenes
from sphere_update import (F, SEED, canonical, jiggle, moved_desc, record_words, shuffle, special_spheres, sph_data)
from test_gpu_mesh_update import FRAMES, dev, frame, oracle_frame, rays_at_the_scene, renderer, same_nodes

pytestmark = pytest.mark.gpu

_DESC, _BUILT = {}, {}
COUNT_EDGES = (40, 64, 65, 128)


def leaf_pairs():
    return (_lib.load().rfx_build_options() >> 8) & 0xFF


def desc_of(key):
    if key not in _DESC:
        _DESC[key] = {"stress33": lambda: scenes.stress_scene(33), "stress100": lambda: scenes.stress_scene(100),
                      "stress300": lambda: scenes.stress_scene(300), "stress4600": lambda: scenes.stress_scene(4600),
                      # the count edges: a full last leaf (no padding lane), a chunk exactly full, one sphere in the last
                      # chunk (tests/test_gpu_tree_limits.py has the same arithmetic at the trees' largest size)
                      **{f"stress{n}": (lambda n=n: scenes.stress_scene(n)) for n in COUNT_EDGES},
                      # more nodes than the bounce kernel's LDS holds (tests/test_gpu_parity.py
                      # test_regrouped_large_scene_equals_unregrouped): the global-memory bounce form
                      "stress_global": lambda: scenes.stress_scene(4400 * leaf_pairs()),
                      "soup38s8": lambda: scenes.soup_scene(38, n_spheres=8),
                      "soup1500s300": lambda: scenes.soup_scene(1500, n_spheres=300)}[key]()
    return _DESC[key]


def built(key):
    """(Scene, Camera) of a case as its description has it, built once (never edited: a test that edits builds its own)"""
    if key not in _BUILT:
        from reflaxman_amd.render import build_scene
        _BUILT[key] = build_scene(desc_of(key))
    return _BUILT[key]


def mirror(scene, S):
    """the host mirror's (boxes, children, mt) -- None without a pair tree -- and chunk bounds at the spheres S"""
    boxes, mt, chunks = scene.sph_bvh_refit(S, widen=True)
    d = scene.sph_bvh_dump()
    return ((boxes, d["children"], mt) if d["nodes"] else None), chunks


def device_state(rr):
    return rr.sph_records(), rr.sph_bvh_nodes(), rr.sph_chunk_bounds(), rr.sph_padding()


def same_state(got, want):
    (rec, nodes, chunks, pad), (wrec, wnodes, wchunks, wpad) = got, want
    return (rec.tobytes() == wrec.tobytes() and chunks.tobytes() == wchunks.tobytes() and pad.tobytes() == wpad.tobytes()
            and ((nodes is None and wnodes is None) or same_nodes(nodes, wnodes)))


# ------------------------------------------------------------------------------------------------ records and nodes
@pytest.mark.parametrize("key", ["stress33", "stress100", "soup38s8"] + [f"stress{n}" for n in COUNT_EDGES])
def test_words_follow_the_host_mirror_and_come_back(key):
    """A -> B -> C -> A (a jiggle, then a shuffle of another jiggle): after every update the records are the edited host
    scene's, the nodes the host refit's (widen = 1) and the chunk bounds the mirror's, bit for bit; the padding lanes
    read back unchanged; back at A everything is what set_scene(A) uploaded"""
    from reflaxman_amd.render import build_scene
    s, _ = built(key)
    edited, _ = build_scene(desc_of(key))
    A = sph_data(desc_of(key))
    n = len(A)
    rr = renderer(s, -1)
    state_a = device_state(rr)
    pad = state_a[3]
    lanes = (-n) % (2 * leaf_pairs()) if n > 32 else n % 2
    assert pad.shape == (lanes, 4) and (pad[:, :3] == 0).all() and (pad[:, 3] == F(-np.inf).view(np.uint32)).all()
    want_nodes, want_chunks = mirror(s, A)
    assert (want_nodes is None) == (n <= 32)
    assert same_state(state_a, (s.sph_records(), want_nodes, want_chunks, pad))
    B, Cs = jiggle(A), shuffle(jiggle(A, seed=5))
    for name, S, form in (("B", B, dev), ("C", Cs, np.asarray)):
        rr.update_spheres(0, form(S))
        edited.setSpheres(0, S)
        want_nodes, want_chunks = mirror(s, S)
        got = device_state(rr)
        assert got[0].tobytes() == edited.sph_records().tobytes() == record_words(S).tobytes(), (key, name)
        assert same_state(got, (edited.sph_records(), want_nodes, want_chunks, pad)), (key, name)
        assert not same_state(got, state_a)
    rr.update_spheres(0, A)  # the host form
    assert same_state(device_state(rr), state_a)
    rr.close()


@pytest.mark.parametrize("n", COUNT_EDGES)
def test_count_edge_frame_after_a_jiggle(n):
    """40, 64, 65 and 128 spheres -- a last leaf with no padding lane, a chunk exactly full, a last chunk of one sphere --
    jiggled: the padding lanes are as many as the count leaves over, and the 32x18 frame is the oracle's"""
    key = f"stress{n}"
    s, cam = built(key)
    desc = desc_of(key)
    S = jiggle(sph_data(desc))
    rr = renderer(s, -1)
    assert rr.sph_padding().shape == ((-n) % (2 * leaf_pairs()), 4) and len(rr.sph_chunk_bounds()) == (n + 63) // 64
    assert rr.accel_info().sph_nodes == (n + 2 * leaf_pairs() - 1) // (2 * leaf_pairs()) - 1
    rr.update_spheres(0, dev(S))
    W, H = 32, 18
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame(key + "_jiggle", moved_desc(desc, S), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


def special_case():
    """stress100 jiggled, with special_spheres over spheres 40 .. 51: (moved spheres, their description)"""
    desc = desc_of("stress100")
    S = jiggle(sph_data(desc))
    Sp = special_spheres(desc.camera[0])
    S[40:40 + len(Sp)] = Sp
    return S, moved_desc(desc, S)


def test_special_spheres():
    """radius 0, -1, 1e-30, NaN, +inf; a NaN and an infinite centre component; centre 1e30; centre 1e15 with radius
    1e14; a sphere enclosing the camera; two coincident spheres (the lower object index wins the tie): the words are the
    mirror's, every NaN as 0x7FC00000, and the 64x36 frame is the oracle's of the moved description"""
    s, cam = built("stress100")
    S, moved = special_case()
    rr = renderer(s, -1)
    rr.update_spheres(0, dev(S))
    want_nodes, want_chunks = mirror(s, S)
    rec, nodes, chunks, _ = device_state(rr)
    assert rec.tobytes() == record_words(S).tobytes()
    assert same_nodes(nodes, want_nodes), [int((a.view(np.uint32) != b.view(np.uint32)).sum())
                                            for a, b in zip(nodes, want_nodes)]
    assert chunks.tobytes() == want_chunks.tobytes()
    assert (canonical(nodes[0]) == nodes[0].view(np.uint32)).all() and np.isnan(nodes[0]).any()
    W, H = 64, 36
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("stress100_special", moved, W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


# ------------------------------------------------------------------------------------------------ frames
@pytest.mark.parametrize("key", ["stress300", "soup1500s300", "soup38s8"])
@pytest.mark.parametrize("W,H,ss,knobs", FRAMES, ids=str)
def test_frames_after_a_jiggle(key, W, H, ss, knobs):
    """centres +- 0.3, radii x [0.8, 1.25] on every sphere (torch tensors): the oracle's frame of the moved scene under
    every schedule knob and sampling mode -- a pair tree and the LDS-staged bounce kernel, both trees, no pair tree"""
    s, cam = built(key)
    desc = desc_of(key)
    S = jiggle(sph_data(desc))
    # (the oracle tests every object for every ray: 256 samples a pixel over 1,800 objects get two segments, not six)
    depth = 2 if key == "soup1500s300" and ss == 16 else 6
    ref = oracle_frame(key + "_jiggle", moved_desc(desc, S), W, H, depth, ss)
    rr = renderer(s, 1 if key == "soup1500s300" else -1, **knobs)
    tri_before = rr.tri_bvh_nodes()
    rr.update_spheres(0, dev(S))
    img = frame(rr, cam, W, H, depth, ss)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    assert (rr.accel_info().sph_nodes > 0) == (key != "soup38s8")
    if key != "soup38s8" and not knobs and ss == 1:
        assert rr.bounce_form() == 2
    if key == "soup1500s300":
        assert rr.accel_info().tri_nodes > 0 and same_nodes(rr.tri_bvh_nodes(), tri_before)  # the triangle tree: untouched
    rr.close()


@pytest.mark.parametrize("key,form", [("stress4600", 2), ("stress_global", 1)])
def test_large_scene_frame_after_a_jiggle(key, form):
    """4,600 spheres, and as many as put the pair tree beyond the bounce kernel's LDS (the global-memory bounce form), at
    32x18: the oracle's frame"""
    s, cam = built(key)
    desc = desc_of(key)
    S = jiggle(sph_data(desc))
    W, H = 32, 18
    ref = oracle_frame(key + "_jiggle", moved_desc(desc, S), W, H, 6)
    rr = renderer(s, -1)
    rr.update_spheres(0, dev(S))
    img = frame(rr, cam, W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    assert rr.bounce_form() == form and rr.accel_info().sph_nodes > 0
    rr.close()


@pytest.mark.parametrize("W,H,ss,knobs", FRAMES, ids=str)
def test_frames_after_a_shuffle(W, H, ss, knobs):
    """the centres permuted among the spheres of stress300: the topology is stale everywhere, the values are the oracle's"""
    s, cam = built("stress300")
    desc = desc_of("stress300")
    S = shuffle(jiggle(sph_data(desc), seed=5))
    ref = oracle_frame("stress300_shuffle", moved_desc(desc, S), W, H, 6, ss)
    rr = renderer(s, -1, **knobs)
    rr.update_spheres(0, S)  # the host form
    img = frame(rr, cam, W, H, 6, ss)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


@pytest.mark.parametrize("form", ["torch", "host"])
def test_ids_update(form):
    """a scattered 10% of stress300's spheres by id, one id out of range: the named spheres move, the others' words are
    untouched, the tree and chunk bounds are the mirror's and the frame is the oracle's"""
    s, cam = built("stress300")
    desc = desc_of("stress300")
    A = sph_data(desc)
    n = len(A)
    rng = np.random.default_rng(21)
    ids = rng.permutation(n)[:n // 10].astype(np.uint32)
    ids[7] = n + 5  # a dead lane
    rec = jiggle(A, seed=8)[np.minimum(ids, n - 1)]
    S = A.copy()
    live = ids < n
    S[ids[live]] = rec[live]
    rr = renderer(s, -1)
    before = rr.sph_records()
    if form == "torch":
        rr.update_spheres(12345, dev(rec), dev(ids.view(np.int32)))  # (`first` is ignored)
    else:
        rr.update_spheres(0, rec, ids)
    after = rr.sph_records()
    changed = np.zeros(n, bool)
    changed[ids[live]] = True
    assert changed.sum() == n // 10 - 1
    assert after[~changed].tobytes() == before[~changed].tobytes()
    assert (after[changed] != before[changed]).any(axis=1).all()
    assert after.tobytes() == record_words(S).tobytes()
    want_nodes, want_chunks = mirror(s, S)
    assert same_nodes(rr.sph_bvh_nodes(), want_nodes) and rr.sph_chunk_bounds().tobytes() == want_chunks.tobytes()
    W, H = 64, 36
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("stress300_ids", moved_desc(desc, S), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


# ------------------------------------------------------------------------------------------------ stream order
def test_update_between_two_frames_on_one_stream():
    """frame, update, frame enqueued on one stream with no host sync between: the first is the oracle's of A, the second
    the oracle's of B from the stream state the first left; the update leaves both random streams alone"""
    import oracle as orc
    import torch
    from reflaxman_amd.render import make_frame
    s, cam = built("stress300")
    desc = desc_of("stress300")
    S = jiggle(sph_data(desc), seed=3)
    W, H, depth = 64, 36, 6
    o1 = orc.OracleRender(desc, SEED, 0)
    o1.set_image_size(W, H)
    o1.render(depth, 1)
    seed1 = o1.sphere_seed.value
    o2 = orc.OracleRender(moved_desc(desc, S), seed1, 0)
    o2.set_image_size(W, H)
    o2.render(depth, 1)
    rr = renderer(s, -1)
    f = make_frame(cam, W, H, depth, 1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_S = dev(S)
        img = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        st.synchronize()  # (the inputs are in place; nothing below waits on the host)
        rr.render_frame(f, img[0].data_ptr(), stream=st.cuda_stream)
        rr.update_spheres(0, d_S)
        rr.render_frame(f, img[1].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert img[0].cpu().numpy().tobytes() == o1.image.tobytes()
    assert img[1].cpu().numpy().tobytes() == o2.image.tobytes()
    # get_rng reads what two frames on a fresh renderer leave
    assert rr.get_rng()[0] == o2.sphere_seed.value
    fresh = renderer(s, -1)
    for _ in range(2):
        frame(fresh, cam, W, H, depth)
    assert fresh.get_rng() == rr.get_rng()
    fresh.close()
    # the streams before and after an update on its own
    rr.set_rng(seed1, 77)
    before = rr.get_rng()
    with torch.cuda.stream(st):
        rr.update_spheres(0, d_S)
    st.synchronize()
    assert rr.get_rng() == before == (seed1, 77)
    rr.close()


# ------------------------------------------------------------------------------------------------ interleaving
def test_interleaved_with_triangle_updates_and_a_recut():
    """update_spheres, update_triangles, recut_triangles and update_spheres again on soup1500s300: the oracle's frame of
    the scene with both moved, and both trees' nodes equal their mirrors"""
    s, cam = built("soup1500s300")
    desc = desc_of("soup1500s300")
    S1, S2 = jiggle(sph_data(desc), seed=1), jiggle(sph_data(desc), seed=2)
    V = wave(tri_vertices(desc), amp=0.4)
    rr = renderer(s, 1)
    rr.update_spheres(0, dev(S1))
    rr.update_triangles(0, dev(V))
    rr.recut_triangles()
    rr.update_spheres(0, S2)
    want_nodes, want_chunks = mirror(s, S2)
    assert same_nodes(rr.sph_bvh_nodes(), want_nodes) and rr.sph_chunk_bounds().tobytes() == want_chunks.tobytes()
    cut = s.tri_bvh_recut(V, widen=True)
    assert same_nodes(rr.tri_bvh_nodes(), (cut["boxes"], cut["children"], cut["mt"]))
    W, H = 48, 27
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("soup1500_both", moved_desc(moved_tris(desc, V), S2), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


# ------------------------------------------------------------------------------------------------ batch calls
def test_batch_calls_equal_a_fresh_renderer():
    """trace_rays plain and in the coherent order, query_hits, occluded, one span call and one paths step on 4,096
    rays: the updated renderer equals a fresh renderer of the moved scene byte for byte, from one stream state; the
    coherent order's key box is the update's to leave alone"""
    from reflaxman_amd.render import build_scene
    desc = desc_of("stress300")
    s, _ = built("stress300")
    S = jiggle(sph_data(desc), seed=4)
    S[0, :3] = (-20.0, 1.0, 0.0)  # (beyond the ground quad: moves the key box of a fresh build)
    edited, _ = build_scene(moved_desc(desc, S))
    rays = rays_at_the_scene(seed=9)
    rr, fresh = renderer(s, -1), renderer(edited, -1)
    box = rr.order_box()
    rr.update_spheres(0, dev(S))
    assert all(np.array_equal(a, b) for a, b in zip(rr.order_box(), box))
    assert not np.array_equal(rr.order_box()[0], fresh.order_box()[0])
    for kw in ({}, {"order": "coherent"}):
        rr.set_rng(SEED, 0)
        fresh.set_rng(SEED, 0)
        a, b = rr.trace_rays(rays, 6, **kw), fresh.trace_rays(rays, 6, **kw)
        assert a.tobytes() == b.tobytes(), kw
        assert rr.get_rng() == fresh.get_rng()
    a, b = rr.query_hits(rays), fresh.query_hits(rays)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["object"] >= 0).sum() > 1000
    assert rr.occluded(rays).tobytes() == fresh.occluded(rays).tobytes()
    lo = np.where(a["object"] < 0, F(np.inf), a["distance"])
    a2, b2 = rr.query_hits(rays, lo=lo, after=a["object"]), fresh.query_hits(rays, lo=lo, after=a["object"])
    for k in a2:
        assert a2[k].tobytes() == b2[k].tobytes(), k
    assert (a2["object"] >= 0).sum() > 100
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
    s, cam = built("stress300")
    desc = desc_of("stress300")
    S = np.ascontiguousarray(jiggle(sph_data(desc)))
    W, H = 64, 36
    g = C.c_void_p()
    _lib.check(L.rfx_group_create(C.byref(g), (C.c_int * 2)(0, 0), 2), "group_create")
    _lib.check(L.rfx_group_set_scene(g, s._h), "group_set_scene")
    for m in range(2):
        _lib.check(L.rfx_renderer_update_spheres_host(C.c_void_p(L.rfx_group_renderer(g, m)), 0, len(S), _lib.fptr(S), None),
                   "update_spheres_host")
    _lib.check(L.rfx_renderer_set_rng(C.c_void_p(L.rfx_group_renderer(g, 0)), SEED, 0))
    one = renderer(s, -1)
    one.update_spheres(0, S)
    f = make_frame(cam, W, H, 6, 1)
    bufs = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    _lib.check(L.rfx_group_render_frame(g, C.byref(f), C.c_void_p(bufs[0].data_ptr()), None, None))
    one.render_frame(f, bufs[1].data_ptr())
    one.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])
    ref = oracle_frame("stress300_jiggle", moved_desc(desc, S), W, H, 6)
    assert bufs[0].cpu().numpy().tobytes() == ref.tobytes()
    L.rfx_group_destroy(g)
    one.close()


def test_errors():
    from reflaxman_amd.render import Renderer, build_scene
    L = _lib.load()
    s, _ = built("stress100")
    n = desc_of("stress100").n_spheres
    v = np.zeros((4, 4), F)
    v[:, 3] = 1
    ids = np.zeros(4, np.uint32)
    p, i = _lib.fptr(v), _lib.u32ptr(ids)
    ARG, STATE = -1, -3
    rr = Renderer(sphere_seed=SEED)
    assert L.rfx_renderer_update_spheres_host(rr._h, 0, 1, p, None) == STATE  # no scene uploaded
    rr.set_scene(s)
    assert L.rfx_renderer_update_spheres_host(None, 0, 1, p, None) == ARG
    assert L.rfx_renderer_update_spheres_host(rr._h, 0, 1, None, None) == ARG
    assert L.rfx_renderer_update_spheres_host(rr._h, 0, 0, p, None) == ARG
    assert L.rfx_renderer_update_spheres_host(rr._h, n - 3, 4, p, None) == ARG
    assert L.rfx_renderer_update_spheres(None, 0, 1, C.c_void_p(16), None, None) == ARG
    assert L.rfx_renderer_update_spheres(rr._h, 0, 4, None, None, None) == ARG
    assert L.rfx_renderer_update_spheres(rr._h, 0, 0, C.c_void_p(16), None, None) == ARG
    assert L.rfx_renderer_update_spheres(rr._h, n, 1, C.c_void_p(16), None, None) == ARG
    assert L.rfx_renderer_update_spheres_host(rr._h, n - 4, 4, p, None) == 0
    assert L.rfx_renderer_update_spheres_host(rr._h, n + 9, 4, p, i) == 0  # with ids `first` is ignored
    small, _ = build_scene(scenes.default_scene())
    rr.set_scene(small)
    assert L.rfx_renderer_update_spheres_host(rr._h, 0, 1, p, None) == STATE
    assert b"rfx_renderer_set_scene" in L.rfx_last_error()
    assert L.rfx_renderer_update_spheres(rr._h, 0, 1, C.c_void_p(16), None, None) == STATE
    assert b"rfx_renderer_set_scene" in L.rfx_last_error()
    assert L.rfx_renderer_sph_records(rr._h, 0, 1, _lib.u32ptr(np.zeros(12, np.uint32))) == ARG
    with pytest.raises(_lib.RfxError):
        rr.update_spheres(0, v[:1])
    rr.close()
