"""Both hierarchies on the device at the size an int16 stack slot bounds and one primitive past it (tests/limit_scenes.py;
the host side is tests/test_tree_limits_host.py): S_max, 32,768 full pair-tree leaves -- the last leaf is INT16_MIN, the
last node 32766, the refit launches 32,768 leaf lanes, no padding lane; S_over, one sphere more -- no pair tree, 4,097
chunks, the last of one sphere; T_max and T_over, the same for the triangle tree.  Frames and traced rays are the
oracle's, hit queries the reference's answers composed in blocks, the moved trees the host mirrors', all bit for bit; a
fresh renderer is never the reference here."""
import numpy as np
import pytest

import limit_scenes as ls
import mesh_sequence as ms
from hits_helpers import PLANES, same_bits
from mesh_update import SEED, wave
from mesh_update import moved_desc as moved_tris
from rays_helpers import oracle_trace
from reflaxman_amd import _lib
from sphere_update import jiggle, moved_desc, record_words, sph_data
from test_gpu_mesh_update import dev, frame, renderer, same_nodes

pytestmark = pytest.mark.gpu

F = np.float32
CASES = ["S_max", "S_over", "T_max", "T_over"]
DEPTH = 4
RFX_ERR_STATE = -3
_ORACLE, _FRAMES, _TRACED = {}, {}, {}


def tri_accel(case):
    return 1 if case[0] == "T" else -1


def oracle_frame(tag, desc, W, H, ss=1):
    """the oracle's frame of `desc` at DEPTH, once per tag (its scene is built once per tag too), read-only; the rows go
    to eight workers -- every random direction is drawn before the rows start, so the frame is the one-worker frame"""
    import oracle as orc
    if tag not in _ORACLE:
        _ORACLE[tag] = orc.OracleRender(desc, SEED, 0)
    k = (tag, W, H, ss)
    if k not in _FRAMES:
        o = _ORACLE[tag]
        o.sphere_seed.value, o.jitter_seed.value = SEED, 0
        o.set_image_size(W, H)
        o.render(DEPTH, ss, nthreads=8)
        img = o.image.copy()
        img.setflags(write=False)
        _FRAMES[k] = img
    return _FRAMES[k]


def same_frame(rr, cam, ref, W, H, ss=1):
    """the renderer's frame from the streams' first state, as the oracle's frames start, against `ref`"""
    rr.set_rng(SEED, 0)
    img = frame(rr, cam, W, H, DEPTH, ss)
    assert img.tobytes() == ref.tobytes(), int((img != ref).any(axis=2).sum())
    return img


def traced(case):
    """(colours, the sphere stream's state after them) of rays_helpers.oracle_trace on the case's rays, once"""
    if case not in _TRACED:
        rgb, end = oracle_trace(ls.desc_of(case), ls.rays_of(case), DEPTH, SEED)
        rgb.setflags(write=False)
        _TRACED[case] = (rgb, end)
    return _TRACED[case]


def assert_planes(got, want, tag):
    for k in PLANES:
        bad = same_bits(got[k], want[k])
        assert bad.size == 0, (tag, k, bad[:8].tolist(), got[k][bad[:2]].tolist(), want[k][bad[:2]].tolist())


# ------------------------------------------------------------------------------------------------ a. the facts of a case
# the last trace launch's bounce kernel (rfx.h rfx_renderer_bounce_form) of a parked 16 x 9 frame: S_max's 32,767 nodes
# are far beyond the LDS-staged kernel's ~2,100, and a scene without a pair tree has nothing to stage -- the
# global-memory form everywhere; no bounce kernel without regrouping
BOUNCE_FORM = {"S_max": 1, "S_over": 1, "T_max": 1, "T_over": 1}


@pytest.mark.parametrize("case", CASES)
def test_facts_and_frames(case):
    """what the case is on the device -- the node counts, no padding lane behind a full last leaf -- and the 16 x 9
    frame with and without regrouping and the 8 x 4 frame at four samples a pixel against the oracle's"""
    s, cam, _ = ls.built(case)
    desc = ls.desc_of(case)
    pairs, tri_leaf = ls.switches()
    rr = renderer(s, tri_accel(case))
    info = rr.accel_info()
    want = {"S_max": (ls.LIMIT_LEAVES - 1, 0), "S_over": (0, 0), "T_max": (0, ls.LIMIT_LEAVES - 1), "T_over": (0, 0)}[case]
    assert (info.sph_nodes, info.tri_nodes) == want, (info.sph_nodes, info.tri_nodes)
    if case == "T_max":
        assert (info.tri_in_leaves, info.tri_residual, info.tri_leaf_size) == (ls.n_t(), 0, tri_leaf)
        assert 0 < info.tri_depth <= 16
    if case == "S_max":
        assert 0 < info.sph_depth <= 16
    pad = rr.sph_padding()
    lanes = {"S_max": 0, "S_over": pairs - 1}.get(case, 0)
    assert pad.shape == (lanes, 4) and (pad[:, :3] == 0).all() and (pad[:, 3] == F(-np.inf).view(np.uint32)).all()
    assert (rr.sph_bvh_nodes() is None) == (info.sph_nodes == 0) and (rr.tri_bvh_nodes() is None) == (info.tri_nodes == 0)
    if case[0] == "S":
        assert len(rr.sph_chunk_bounds()) == (desc.n_spheres + 63) // 64
    same_frame(rr, cam, oracle_frame(case, desc, 16, 9), 16, 9)
    print(case, "bounce form", rr.bounce_form())
    assert rr.bounce_form() == BOUNCE_FORM[case]
    same_frame(rr, cam, oracle_frame(case, desc, 8, 4, 4), 8, 4, 4)
    rr.close()
    rr = renderer(s, tri_accel(case), regroup=0)
    same_frame(rr, cam, oracle_frame(case, desc, 16, 9), 16, 9)
    assert rr.bounce_form() == 0
    rr.close()


# ------------------------------------------------------------------------------------------------ c. batch calls
@pytest.mark.parametrize("case", CASES)
def test_batch_calls(case):
    """256 rays -- 128 through the scene, 128 aimed at primitives of leaf 0, of the last leaf, of the leaves under the
    last node and of leaves drawn with a fixed seed: query_hits (all six planes), occluded and one next-hit layer against
    the reference composed in blocks; trace_rays, plain and in the coherent order, against the oracle"""
    s, _, _ = ls.built(case)
    desc = ls.desc_of(case)
    rays = ls.rays_of(case)
    want, occ = ls.composed(case)
    rr = renderer(s, tri_accel(case))
    got = rr.query_hits(np.array(rays))
    assert_planes(got, want, case)
    # the closest hits reach the corners of the tree (the no-tree cases: the same primitives, through the chunk loops)
    prims, named = ls.targets(case)
    obj = ls.prim_objects(desc, "sphere" if case[0] == "S" else "triangle")
    for k in ("first", "last", "under_last_node"):
        assert np.isin(got["object"], obj[named[k]]).any(), k
    assert (got["object"][ls.N_RAYS:] == obj[prims]).sum() >= 64
    assert rr.occluded(np.array(rays)).tobytes() == occ.tobytes()
    lo = np.where(want["object"] < 0, F(np.inf), want["distance"])
    behind = rr.query_hits(np.array(rays), lo=lo, after=np.array(want["object"]))
    assert_planes(behind, ls.composed(case, 1)[0], case + " layer 1")
    assert (behind["object"] >= 0).sum() > 64
    rgb, end = traced(case)
    for kw in ({}, {"order": "coherent"}):
        rr.set_rng(SEED, 0)
        out = rr.trace_rays(np.array(rays), DEPTH, **kw)
        assert out.tobytes() == rgb.tobytes(), (kw, same_bits(out, rgb)[:8].tolist())
        assert rr.get_rng() == (end, 0)
    rr.close()


# ------------------------------------------------------------------------------------------------ d. moving at the limit
def sphere_mirror(scene, S):
    boxes, mt, chunks = scene.sph_bvh_refit(S, widen=True)
    d = scene.sph_bvh_dump()
    return ((boxes, d["children"], mt) if d["nodes"] else None), chunks


def assert_sphere_state(rr, s, S, tag):
    """records, nodes (all of them) and chunk bounds of the renderer against the host mirror at the spheres S"""
    want_nodes, want_chunks = sphere_mirror(s, S)
    assert rr.sph_records().tobytes() == record_words(S).tobytes(), tag
    got = rr.sph_bvh_nodes()
    if want_nodes is None:
        assert got is None, tag
    else:
        assert len(got[0]) == len(want_nodes[0]) and same_nodes(got, want_nodes), \
            (tag, [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(got, want_nodes)])
    chunks = rr.sph_chunk_bounds()
    assert chunks.tobytes() == want_chunks.tobytes(), (tag, np.flatnonzero((chunks != want_chunks).any(axis=1))[:8].tolist())
    return chunks


def test_moving_spheres_at_the_limit():
    """every sphere of S_max jiggled (torch tensors): all 32,767 nodes, the chunk bounds and the records are the
    mirror's and the frame the oracle's of the moved scene; then the last leaf's spheres alone by id with one dead id;
    then back through the host form to what set_scene left"""
    s, cam, d = ls.built("S_max")
    desc = ls.desc_of("S_max")
    A = sph_data(desc)
    n = len(A)
    rr = renderer(s, -1)
    state_a = (rr.sph_records(), rr.sph_bvh_nodes(), rr.sph_chunk_bounds())
    assert len(state_a[1][0]) == ls.LIMIT_LEAVES - 1
    assert_sphere_state(rr, s, A, "A")
    B = jiggle(A)
    rr.update_spheres(0, dev(B))
    assert_sphere_state(rr, s, B, "B")
    assert not same_nodes(rr.sph_bvh_nodes(), state_a[1])
    same_frame(rr, cam, oracle_frame("S_max_jiggle", moved_desc(desc, B), 16, 9), 16, 9)
    # the last leaf's spheres, and one id that names no sphere
    last = np.array(ls.leaf_prims(d, ls.LIMIT_LEAVES - 1), np.uint32)
    ids = np.concatenate([last[:3], [n + 5], last[3:]]).astype(np.uint32)
    rec = jiggle(B, seed=8)[np.minimum(ids, n - 1)]
    Cs = B.copy()
    Cs[last] = rec[ids < n]
    before = rr.sph_records()
    rr.update_spheres(12345, dev(rec), dev(ids.view(np.int32)))  # (`first` is ignored)
    after = rr.sph_records()
    changed = np.zeros(n, bool)
    changed[last] = True
    assert after[~changed].tobytes() == before[~changed].tobytes() and (after[changed] != before[changed]).any(axis=1).all()
    assert_sphere_state(rr, s, Cs, "ids")
    same_frame(rr, cam, oracle_frame("S_max_ids", moved_desc(desc, Cs), 16, 9), 16, 9)
    rr.update_spheres(0, A)  # the host form
    got = (rr.sph_records(), rr.sph_bvh_nodes(), rr.sph_chunk_bounds())
    assert got[0].tobytes() == state_a[0].tobytes() and same_nodes(got[1], state_a[1]) and got[2].tobytes() == state_a[2].tobytes()
    rr.close()


def test_moving_spheres_past_the_limit():
    """S_over jiggled: no pair tree (rfx_update.cpp's refit stops at the chunks), 4,097 chunk bounds equal to the
    mirror's, the last of one sphere, and the oracle's frame; then that one sphere alone by id moves its chunk's bound and
    no other"""
    s, cam, d = ls.built("S_over")
    desc = ls.desc_of("S_over")
    A = sph_data(desc)
    n = len(A)
    chunks = ls.n_s() // 64 + 1
    rr = renderer(s, -1)
    B = jiggle(A)
    rr.update_spheres(0, dev(B))
    got = assert_sphere_state(rr, s, B, "B")
    assert rr.sph_bvh_nodes() is None and got.shape == (chunks, 4)
    dev_index = d["device_index"]
    alone = np.flatnonzero(dev_index // 64 == chunks - 1)
    assert len(alone) == 1
    same_frame(rr, cam, oracle_frame("S_over_jiggle", moved_desc(desc, B), 16, 9), 16, 9)
    Cs = B.copy()
    Cs[alone[0]] = (B[alone[0]] + F([0.25, 0.0, -0.25, 0.01])).astype(F)
    rr.update_spheres(0, dev(Cs[alone]), dev(alone.astype(np.int32)))
    after = assert_sphere_state(rr, s, Cs, "ids")
    assert after[:-1].tobytes() == got[:-1].tobytes() and after[-1].tobytes() != got[-1].tobytes()
    rr.close()


def test_moving_triangles_at_the_limit():
    """a height wave on every vertex of T_max: the nodes are the host refit's and the frame the oracle's; re-cut, the
    nodes, the leaves' triangles, the slot map and the depth are the host re-cut's and the frame stays, bit for bit"""
    s, cam, d = ls.built("T_max")
    desc = ls.desc_of("T_max")
    V = wave(ls.triangle_rows(desc))
    rr = renderer(s, 1)
    rr.update_triangles(0, dev(V))
    boxes, mt = s.tri_bvh_refit(V, widen=True)
    got = rr.tri_bvh_nodes()
    assert len(got[0]) == ls.LIMIT_LEAVES - 1 and same_nodes(got, (boxes, d["children"], mt)), \
        [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(got, (boxes, d["children"], mt))]
    ref = oracle_frame("T_max_wave", moved_tris(desc, V), 16, 9)
    img = same_frame(rr, cam, ref, 16, 9)
    rr.recut_triangles()
    cut = s.tri_bvh_recut(V, widen=True)
    got = rr.tri_bvh_nodes()
    assert same_nodes(got, (cut["boxes"], cut["children"], cut["mt"])), \
        [int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(got, (cut["boxes"], cut["children"], cut["mt"]))]
    assert not np.array_equal(cut["children"], d["children"])
    ids, slot, _ = rr.tri_leaves()
    assert np.array_equal(ids, cut["leaf_ids"]) and np.array_equal(slot, ms.slots_of(cut["leaf_ids"], len(V)))
    assert (slot >= 0).all() and rr.accel_info().tri_depth == cut["depth"] and rr.accel_info().tri_nodes == ls.LIMIT_LEAVES - 1
    assert same_frame(rr, cam, ref, 16, 9).tobytes() == img.tobytes()
    rr.close()


def test_moving_triangles_past_the_limit():
    """T_over: the last 40 triangles of chunk 2,047 and the one triangle of chunk 2,048 -- the one in front of the camera
    -- moved in one range: the oracle's frame through the chunk loops, another frame than before the move; and no re-cut
    without a tree"""
    s, cam, d = ls.built("T_over")
    desc = ls.desc_of("T_over")
    assert d is None
    A = ls.triangle_rows(desc)
    first, count = len(A) - 41, 41
    assert first // 64 == 2047 and (first + count - 1) // 64 == 2048 and len(A) == 64 * 2048 + 1
    V = A.copy()
    V[first:first + count] = wave(A[first:first + count], amp=0.6, phase=0.5)
    rr = renderer(s, 1)
    assert rr.accel_info().tri_nodes == 0 and rr.tri_bvh_nodes() is None
    rr.update_triangles(first, dev(V[first:first + count]))
    ref = oracle_frame("T_over_wave", moved_tris(desc, V), 16, 9)
    assert ref.tobytes() != oracle_frame("T_over", desc, 16, 9).tobytes()
    same_frame(rr, cam, ref, 16, 9)
    assert _lib.load().rfx_renderer_recut_triangles(rr._h, None) == RFX_ERR_STATE
    rr.close()
