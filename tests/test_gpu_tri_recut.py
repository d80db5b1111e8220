"""Re-cutting on the device (rfx.h "Re-cutting", rfx_renderer_recut_triangles): the re-cut tree and the leaf records
bit for bit against the host mirror, and -- the values contract -- frames of every mode against the oracle of the moved
scene and the batch calls against a fresh renderer's, after a shuffle that takes the mesh out of the shape its tree was
cut at."""
import ctypes as C

import numpy as np
import pytest

import recut_helpers as rh
from mesh_update import F, SEED, moved_desc, tri_vertices, wave
from reflaxman_amd import _lib, scenes
from test_gpu_mesh_update import built, desc_of, dev, frame, make_ill, oracle_frame, rays_at_the_scene, renderer, same_nodes

pytestmark = pytest.mark.gpu

_BIG = {}


def case(key):
    """(description, built Scene, camera) of a case; soup4200 (more in-tree triangles than the sort's tile) and the leaf-count
    edges soup63 and soup64 (tests/test_tri_recut_host.py test_leaf_edges) are this file's"""
    own = {"soup4200": 4200, "soup63": 61, "soup64": 62}  # (the soup's two ground triangles come on top)
    if key not in own:
        return (desc_of(key), *built(key))
    if key not in _BIG:
        from reflaxman_amd.render import build_scene
        desc = scenes.soup_scene(own[key])
        _BIG[key] = (desc, *build_scene(desc))
    return _BIG[key]


def mirror_nodes(s, cut, fit=None):
    r = s.tri_bvh_recut(cut, fit, widen=True)
    return r["boxes"], r["children"], r["mt"]


def check_records(rr, desc, V):
    """the device's words are the host scene's edited to V, and the tree's copy is the triangle's own record"""
    from reflaxman_amd.render import build_scene
    edited, _ = build_scene(desc)
    edited.setTriangleVertices(0, V)
    got, want = rr.tri_records(), edited.tri_records()
    assert got[:, :29].tobytes() == want[:, :29].tobytes()
    assert got[:, 29:41].tobytes() == got[:, 0:12].tobytes()


# ------------------------------------------------------------------------------------------------ nodes and records
@pytest.mark.parametrize("key", ["mesh", "degenerate", "soup33", "soup4200", "soup63", "soup64"])
def test_nodes_equal_the_mirror_and_stay_in_step(key):
    desc, s, _ = case(key)
    V = tri_vertices(desc)
    rr = renderer(s, 1)
    info = rr.accel_info()
    nodes0 = rr.tri_bvh_nodes()
    S = rh.shuffle(V)
    rr.update_triangles(0, dev(S))
    stale = rr.tri_bvh_nodes()
    rr.recut_triangles()
    got, want = rr.tri_bvh_nodes(), mirror_nodes(s, S)
    assert same_nodes(got, want), [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(got, want)]
    assert not np.array_equal(got[1], nodes0[1]) and not same_nodes(got, stale)
    check_records(rr, desc, S)
    after = rr.accel_info()
    G = -(-(len(V) - info.tri_residual) // rh.LEAF)
    assert after.tri_nodes == info.tri_nodes == G - 1 and after.tri_depth == (G - 1).bit_length()
    assert (after.tri_in_leaves, after.tri_residual) == (info.tri_in_leaves, info.tri_residual)
    # an update after the re-cut works on the new slots, order and height lists
    second = wave(rh.shuffle(V, amp=3.0, seed=7), amp=0.5)
    rr.update_triangles(0, dev(second))
    got, want = rr.tri_bvh_nodes(), mirror_nodes(s, S, second)
    assert same_nodes(got, want), [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(got, want)]
    check_records(rr, desc, second)
    # twice at the same vertices: identical, and the mirror's cut at them
    rr.recut_triangles()
    a = rr.tri_bvh_nodes()
    rr.recut_triangles()
    b = rr.tri_bvh_nodes()
    assert same_nodes(a, b) and same_nodes(a, mirror_nodes(s, second))
    check_records(rr, desc, second)
    rr.close()


# ------------------------------------------------------------------------------------------------ degenerate cuts
def degenerate_cuts():
    """{case: (X, placed, ill)}: the vertex sets of tests/test_tri_recut_host.py's box edge cases and the ones only the
    device's box reduction can get wrong -- an empty box, one and two placed triangles, an extent that overflows, a
    non-finite sum from finite vertices -- with the placed and ill counts of the restatement on the CPU"""
    if "cuts" not in _BIG:
        V = tri_vertices(case("mesh")[0])
        n = len(V)
        S = rh.shuffle(V)
        c = {"same": (np.broadcast_to(V[5], V.shape).copy(), n, 0)}
        flat = V.copy()
        flat[..., 1] = 0.0
        c["flat"] = (flat, n, 0)
        for tag, pick in (("even", slice(0, None, 2)), ("first", slice(0, 1)), ("all", slice(None))):
            signed = flat.copy()
            signed[pick, :, 1] = -0.0
            c["signed_zero_" + tag] = (signed, n, 0)
        step = flat.copy()
        step[::3, :, 1] = 4.0
        step[1::3, :, 1] = -0.0
        c["zero_bound"] = (step, n, 0)
        far = S.copy()
        far[0::2, :, 0] += F(1e38)
        far[1::2, :, 0] -= F(1e38)
        c["overflow_extent"] = (far, 344, 40)
        inf = S.copy()
        inf[7, :, 2] = 2e38
        c["inf_sum"] = (inf, n - 1, 0)
        ill = S.copy()
        ill[:, 2] = ill[:, 1]
        c["all_ill"] = (ill, 0, n)
        one = ill.copy()
        one[100] = S[100]
        c["one_placed"] = (one, 1, n - 1)
        two = one.copy()
        two[300] = S[300]
        c["two_placed"] = (two, 2, n - 2)
        _BIG["cuts"] = c
    return _BIG["cuts"]


CUTS = ["same", "flat", "signed_zero_even", "signed_zero_first", "signed_zero_all", "zero_bound", "overflow_extent",
        "inf_sum", "all_ill", "one_placed", "two_placed"]
# the mesh is out of the 4,096 rays' reach in overflow_extent (x = +-1e38): they hit the eight spheres alone, 341 times
# by the reference composed on the CPU (hits_helpers.compose), so that case's full check asks for 300 hits, not 1,000
FULL = {"all_ill": 1000, "one_placed": 1000, "overflow_extent": 300}


@pytest.mark.parametrize("name", CUTS)
def test_degenerate_cuts_equal_the_mirror(name):
    """update to X, re-cut: the tree, membership, slots and leaf records are the host mirror's and the float32
    restatement's, where the device's integer box reduction and the host's fminf / fmaxf fold take different roads; a tree
    that is all NaN spines still gives a fresh renderer's words"""
    import mesh_sequence as ms
    from test_gpu_mesh_sequences import cheap_checks, full_check
    X, placed, ill = degenerate_cuts()[name]
    m = ms.Model("mesh")
    classes = rh.classes(m.desc, X)
    want = rh.restated(X, classes, m.tree)
    assert (int(want["placed"].sum()), int(classes.sum())) == (placed, ill)
    keys = want["keys"]
    if name in ("same", "one_placed", "overflow_extent"):
        assert want["scale"] == 0 and set(keys[want["placed"]].tolist()) == {0}
    if name == "same":
        assert np.array_equal(want["leaf_ids"].reshape(-1), m.tree)  # one key: index order
    if name == "flat" or name.startswith("signed_zero"):
        assert (keys & 0x12492492).sum() == 0 and want["scale"] > 0  # no y bit in any key
        assert np.array_equal(want["leaf_ids"], rh.restated(degenerate_cuts()["flat"][0], classes, m.tree)["leaf_ids"])
    if name == "zero_bound":
        assert want["lo"][1] == 0 and want["hi"][1] == 12 and (keys & 0x12492492).any()
    if name == "inf_sum":
        assert classes[7] == 0 and not want["placed"][7] and keys[7] == rh.LAST_KEY  # well-conditioned, and not placed
    if name == "all_ill":
        assert want["lo"] is None and (keys == rh.LAST_KEY).all()
    if name == "two_placed":
        assert abs(float(want["scale"]) - 17.02) < 0.01
    rr = renderer(m.scene, 1)
    i = rr.accel_info()
    info0 = (i.tri_nodes, i.tri_residual, i.tri_in_leaves)
    rr.update_triangles(0, dev(X))
    rr.recut_triangles()
    m.apply(ms.Op("whole", 0, X))
    m.apply(ms.Op("recut"))
    e = m.expected()  # (scene.tri_bvh_recut(X, widen=True), and the records of the Scene edited to X)
    assert np.array_equal(e["leaf_ids"], want["leaf_ids"]) and np.array_equal(e["children"], want["children"])
    nan = int(np.isnan(e["boxes"]).any(axis=2).sum())
    assert nan == {"overflow_extent": 23, "all_ill": 190, "one_placed": 190, "two_placed": 190}.get(name, 0), nan
    cheap_checks(rr, m, e, info0, name)
    assert np.array_equal(rr.tri_leaves()[0], want["leaf_ids"])
    if name in FULL:
        full_check(rr, m.desc, X, name, min_hits=FULL[name])
    rr.close()


# ------------------------------------------------------------------------------------------------ frames
FRAMES = [(64, 36, 1, {}), (64, 36, 1, {"regroup": 0}), (64, 36, 1, {"regroup": 1}), (64, 36, 1, {"launch_traces": 500}),
          (32, 18, 4, {}), (16, 9, 16, {}), (48, 27, -3, {})]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("W,H,ss,knobs", FRAMES, ids=str)
def test_mesh_frames_after_a_shuffle_and_a_recut(mode, W, H, ss, knobs):
    desc, s, cam = case("mesh")
    S = rh.shuffle(tri_vertices(desc))
    ref = oracle_frame("mesh_shuffle", moved_desc(desc, S), W, H, 6, ss)
    rr = renderer(s, mode, **knobs)
    rr.update_triangles(0, dev(S))
    rr.recut_triangles()
    img = frame(rr, cam, W, H, 6, ss)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


def test_degenerate_frame_with_ill_triangles_in_the_last_leaves():
    desc, s, cam = case("degenerate")
    ids = s.tri_bvh_dump()["leaf_ids"]
    six = [int(t) for t in ids[[0, 3, 17, 30, 41, 55], 0]]
    V = make_ill(rh.shuffle(tri_vertices(desc), amp=2.0), six)
    rr = renderer(s, 1)
    rr.update_triangles(0, dev(V))
    rr.recut_triangles()
    boxes, kids, _ = rr.tri_bvh_nodes()
    assert same_nodes((boxes, kids), mirror_nodes(s, V)[:2])
    assert np.isnan(boxes[0, 1]).all() and np.isfinite(boxes[0, 0]).all()  # the last leaves are under the root's right
    W, H = 48, 27
    img = frame(rr, cam, W, H, 6)
    ref = oracle_frame("degenerate_ill_recut", moved_desc(desc, V), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


def test_both_trees_parked_frame():
    desc, s, cam = case("soup1500s300")
    S = rh.shuffle(tri_vertices(desc), amp=3.0)
    rr = renderer(s, 1)
    rr.update_triangles(0, dev(S))
    rr.recut_triangles()
    assert same_nodes(rr.tri_bvh_nodes(), mirror_nodes(s, S))
    W, H = 48, 27
    img = frame(rr, cam, W, H, 6)
    assert rr.bounce_form() == 2 and rr.accel_info().sph_nodes > 0
    ref = oracle_frame("soup1500_shuffle", moved_desc(desc, S), W, H, 6)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    rr.close()


# ------------------------------------------------------------------------------------------------ batch calls
def test_batch_calls_equal_a_fresh_renderer():
    """trace_rays and its coherent order, query_hits, occluded, a span form and paths stepped to depth 3 on 4,096 rays:
    word for word a fresh renderer's of the moved scene; the re-cut leaves both random streams alone"""
    from reflaxman_amd.render import build_scene
    desc, s, _ = case("soup300")
    S = rh.shuffle(tri_vertices(desc))
    edited, _ = build_scene(moved_desc(desc, S))
    rays = rays_at_the_scene(seed=9)
    rr, fresh = renderer(s, 1), renderer(edited, 1)
    rr.update_triangles(0, dev(S))
    rr.set_rng(SEED, 77)
    rr.recut_triangles()
    assert rr.get_rng() == (SEED, 77)
    for kw in ({}, {"order": "coherent"}):
        rr.set_rng(SEED, 0)
        fresh.set_rng(SEED, 0)
        a, b = rr.trace_rays(rays, 6, **kw), fresh.trace_rays(rays, 6, **kw)
        assert a.tobytes() == b.tobytes(), kw
        assert rr.get_rng() == fresh.get_rng()
        qa, qb = rr.query_hits(rays, **kw), fresh.query_hits(rays, **kw)
        for k in qa:
            assert qa[k].tobytes() == qb[k].tobytes(), (k, kw)
        assert rr.occluded(rays, **kw).tobytes() == fresh.occluded(rays, **kw).tobytes()
    assert (qa["object"] >= 0).sum() > 1000
    lo = np.where(qa["object"] < 0, F(np.inf), qa["distance"])
    a2, b2 = rr.query_hits(rays, lo=lo, after=qa["object"]), fresh.query_hits(rays, lo=lo, after=qb["object"])
    for k in a2:
        assert a2[k].tobytes() == b2[k].tobytes(), k
    assert (a2["object"] >= 0).sum() > 300
    rr.set_rng(SEED, 0)
    fresh.set_rng(SEED, 0)
    pa, pb = rr.paths(rays), fresh.paths(rays)
    for upto in (1, 2, 3):
        pa.step(upto)
        pb.step(upto)
        for k in ("rays", "mul", "colour", "state"):
            assert getattr(pa, k).tobytes() == getattr(pb, k).tobytes(), (k, upto)
    pa.close()
    pb.close()
    rr.close()
    fresh.close()


def test_frame_update_recut_frame_on_one_stream():
    """frame, update, re-cut, frame enqueued on one stream with device tensors and no host sync between: the first is the
    old scene's, the second the moved scene's from the stream state the first left"""
    import oracle as orc
    import torch
    from reflaxman_amd.render import make_frame
    desc, s, cam = case("mesh")
    S = rh.shuffle(tri_vertices(desc), seed=23)
    W, H, depth = 64, 36, 6
    o1 = orc.OracleRender(desc, SEED, 0)
    o1.set_image_size(W, H)
    o1.render(depth, 1)
    o2 = orc.OracleRender(moved_desc(desc, S), o1.sphere_seed.value, 0)
    o2.set_image_size(W, H)
    o2.render(depth, 1)
    rr = renderer(s, 1)
    f = make_frame(cam, W, H, depth, 1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_S = dev(S)
        img = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        st.synchronize()  # (the inputs are in place; nothing below waits on the host)
        rr.render_frame(f, img[0].data_ptr(), stream=st.cuda_stream)
        rr.update_triangles(0, d_S)
        rr.recut_triangles(stream=st.cuda_stream)
        rr.render_frame(f, img[1].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert img[0].cpu().numpy().tobytes() == o1.image.tobytes()
    assert img[1].cpu().numpy().tobytes() == o2.image.tobytes()
    assert rr.get_rng()[0] == o2.sphere_seed.value
    assert same_nodes(rr.tri_bvh_nodes(), mirror_nodes(s, S))
    rr.close()


def test_two_member_group_after_updates_and_recuts():
    """a device group of two members on device 0, the update and the re-cut on both members' renderers: the group's
    frame is the single renderer's and the oracle's"""
    import torch
    from reflaxman_amd.render import make_frame
    L = _lib.load()
    desc, s, cam = case("mesh")
    S = np.ascontiguousarray(rh.shuffle(tri_vertices(desc)))
    W, H = 64, 36
    g = C.c_void_p()
    _lib.check(L.rfx_group_create(C.byref(g), (C.c_int * 2)(0, 0), 2), "group_create")
    for m in range(2):
        _lib.check(L.rfx_renderer_set_tri_accel(C.c_void_p(L.rfx_group_renderer(g, m)), 1))
    _lib.check(L.rfx_group_set_scene(g, s._h), "group_set_scene")
    for m in range(2):
        member = C.c_void_p(L.rfx_group_renderer(g, m))
        _lib.check(L.rfx_renderer_update_triangles_host(member, 0, len(S), _lib.fptr(S), 3 * len(S), None), "update_triangles_host")
        _lib.check(L.rfx_renderer_recut_triangles(member, None), "recut_triangles")
    _lib.check(L.rfx_renderer_set_rng(C.c_void_p(L.rfx_group_renderer(g, 0)), SEED, 0))
    one = renderer(s, 1)
    one.update_triangles(0, S)
    one.recut_triangles()
    f = make_frame(cam, W, H, 6, 1)
    bufs = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    _lib.check(L.rfx_group_render_frame(g, C.byref(f), C.c_void_p(bufs[0].data_ptr()), None, None))
    one.render_frame(f, bufs[1].data_ptr())
    one.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])
    ref = oracle_frame("mesh_shuffle", moved_desc(desc, S), W, H, 6)
    assert bufs[0].cpu().numpy().tobytes() == ref.tobytes()
    L.rfx_group_destroy(g)
    one.close()


def test_errors():
    from reflaxman_amd.render import Renderer, build_scene
    L = _lib.load()
    ARG, STATE = -1, -3
    _, s, _ = case("mesh")
    assert L.rfx_renderer_recut_triangles(None, None) == ARG
    rr = Renderer(sphere_seed=SEED)
    assert L.rfx_renderer_recut_triangles(rr._h, None) == STATE  # no scene uploaded
    small, _ = build_scene(scenes.default_scene())
    rr.set_scene(small)
    assert L.rfx_renderer_recut_triangles(rr._h, None) == STATE
    rr.set_tri_accel(0)
    rr.set_scene(s)
    assert rr.accel_info().tri_nodes == 0
    assert L.rfx_renderer_recut_triangles(rr._h, None) == STATE
    assert b"triangle tree" in L.rfx_last_error()
    with pytest.raises(_lib.RfxError):
        rr.recut_triangles()
    rr.close()
    rr = renderer(s, 1)
    assert L.rfx_renderer_recut_triangles(rr._h, None) == 0  # at the vertices set_scene uploaded
    rr.close()
