"""The coherent order on the GPU (rfx.h rfx_rays_order and the ordered calls): the device keys against their numpy
restatement (order_helpers), the sort against the stable argsort of those keys, and the ordered trace and queries
against the CPU references of the unordered calls (rays_helpers.incoherent_oracle, hits_helpers.compose).  The bar is
bit equality everywhere: an order moves work between waves and changes no word."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
import order_helpers as oh
from helpers import GOLDEN, manifest
from hits_helpers import PLANES, any_hit, compose, same_bits
from rays_helpers import DEPTH, NRAYS, SEED, incoherent_oracle, incoherent_rays, scene
from reflaxman_amd import _lib, cameras, scenes

pytestmark = pytest.mark.gpu

RFX_ERR_ARG, RFX_ERR_STATE = -1, -3
T = _lib.RFX_ORDER_TILE
SENT, PAD = 0x5A5A5A5A, 64
_DESC = {}


def desc_of(name):
    """A scene description by name: rays_helpers' scenes, and the ones only these tests use (test_gpu_hits.py's)."""
    if name not in _DESC:
        if name == "soup300_degenerate":
            _DESC[name] = scenes.degenerate_soup_scene()
        elif name == "mesh100_plane":  # a triangle tree and a plane in one scene
            d = scenes.get_scene("mesh100")
            d.add_plane((0.0, -0.05, 0.0), (0.0, 2.0, 0.0), scenes.DIELECTRIC, (0.8, 0.85, 0.9), 0.6)
            _DESC[name] = d
        elif name == "plane_only":  # nothing the key's box counts
            d = scenes.SceneDesc("plane_only", (0.9, 0.9, 1.0, 0.1), ((0.0, 3.0, -8.0), (0.0, 0.5, 0.0), 1.0))
            d.add_plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.METAL, (1.0, 0.0, 1.0), 0.5)
            _DESC[name] = d
        else:
            _DESC[name] = scene(name)
    return _DESC[name]


def renderer(name, tri_accel=None, seed=SEED):
    """(Renderer with the scene uploaded, its Scene -- kept alive by the caller --, the scene's Camera)."""
    from reflaxman_amd.render import Renderer, build_scene
    s, cam = build_scene(desc_of(name))
    r = Renderer(sphere_seed=seed, jitter_seed=77)
    if tri_accel is not None:
        r.set_tri_accel(tri_accel)
    r.set_scene(s)
    return r, s, cam


def dev(a):
    import torch
    a = np.array(a)  # (a copy: the shared references are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def side_stream(fn):
    """fn() on a side stream of torch's, synchronised."""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        out = fn()
        torch.cuda.current_stream().synchronize()
    return out


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def device_order(r, rays, keys=False):
    out = side_stream(lambda: r.order_rays(dev(rays), keys=keys))
    return (u32(out[0]), u32(out[1])) if keys else u32(out)


def pinhole(name, W, H):
    eye, at, fov = desc_of(name).camera
    return cameras.pinhole_rays(eye, orc.camera_view(eye, at), fov, W, H)


def repeated_rays(n):
    """n rays whose keys repeat heavily across the sort's workgroups: a 40 x 24 pinhole frame's rays of the default
    scene over and over, each copy's origins a little further along x."""
    base = pinhole("default", 40, 24)
    i = np.arange(n)
    rays = base[i % len(base)].copy()
    rays[:, 0] += (i // len(base)).astype(np.float32) * np.float32(1e-3)
    return rays


def fixed_permutation(n):
    return np.random.default_rng(12).permutation(n).astype(np.uint32)


# ------------------------------------------------------------------ 1. keys
def extremes(desc):
    """Per sphere and per triangle vertex of a description, its least and greatest point per axis, in float32."""
    mins, maxs = [], []
    for ob in desc.objects:
        if ob[0] == "sphere":
            c, rad = np.asarray(ob[1], np.float32), np.float32(ob[2])
            mins.append(c - rad)
            maxs.append(c + rad)
        elif ob[0] == "triangle":
            for v in ob[1:4]:
                mins.append(np.asarray(v, np.float32))
                maxs.append(np.asarray(v, np.float32))
    return np.array(mins, np.float32), np.array(maxs, np.float32)


@pytest.mark.parametrize("name", ["default", "planes", "stress4096", "mesh40x32", "plane_only"])
def test_keys_equal_the_restatement(name):
    """The device keys of 357 incoherent rays and of the rays at the key's edges equal the numpy float32 restatement
    bit for bit, fed the box the library reports; that box is the description's (planes ignored) and encloses every
    sphere and vertex."""
    d = desc_of(name)
    r, s, cam = renderer(name)
    lo, scale = r.order_box()
    want_lo, want_scale = oh.scene_box(d)
    assert lo.tobytes() == want_lo.tobytes() and scale.tobytes() == want_scale.tobytes(), (name, lo, scale)
    if name == "plane_only":
        assert not scale.any() and not lo.any()
        rays = np.concatenate([incoherent_rays("default"), oh.special_rays()])
    else:
        mins, maxs = extremes(d)
        assert (scale > 0).all() and (lo <= mins).all() and ((maxs - lo) * scale <= (1 << oh.CB) * (1 + 1e-6)).all()
        rays = np.concatenate([incoherent_rays(name), oh.special_rays(lo, maxs.max(axis=0))])
    order, keys = device_order(r, rays, keys=True)
    want = oh.keys(rays, lo, scale)
    bad = np.flatnonzero(keys != want)
    assert bad.size == 0, (name, bad[:8].tolist(), keys[bad[:4]].tolist(), want[bad[:4]].tolist(), rays[bad[:2]].tolist())
    if name == "plane_only":
        assert (keys >> np.uint32(2 * oh.DB) == 0).all()  # scale 0: every cell 0
    else:
        assert len(set((keys >> np.uint32(2 * oh.DB)).tolist())) >= 32  # (the incoherent origins fill the box)
    assert np.array_equal(order, oh.order(want)), name
    # the host form gives the same words
    h_order, h_keys = r.order_rays(rays, keys=True)
    assert h_order.dtype == np.uint32 and np.array_equal(h_order, order) and np.array_equal(h_keys, keys)
    r.close()


# ------------------------------------------------------------------ 2. the sort
def check_sort(r, rays, tag):
    order, keys = device_order(r, rays, keys=True)
    lo, scale = r.order_box()
    assert np.array_equal(keys, oh.keys(rays, lo, scale)), tag
    want = oh.order(keys)
    bad = np.flatnonzero(order != want)
    assert bad.size == 0, (tag, len(rays), bad[:8].tolist(), order[bad[:8]].tolist(), want[bad[:8]].tolist())
    return order, keys


def test_order_is_the_stable_argsort_of_the_keys():
    """Whole-array equality at every size where the sort's path changes (a wave, the workgroup's tile T, several
    workgroups), on one renderer whose scratch is reused and regrown (a smaller n, then a larger one, again)."""
    r, s, cam = renderer("default")
    rays = repeated_rays(100003)
    for n in (357, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 65, 100003, 3 * T + 5, T + 1):
        order, keys = check_sort(r, rays[:n], ("repeated", n))
        if n >= T:
            assert len(set(keys.tolist())) < n // 2  # keys repeat heavily
    inc = incoherent_rays("default")
    check_sort(r, inc, "incoherent")
    r.close()


# Past 256 workgroups order_scan_kernel walks a digit's row of per-workgroup counts in more than one chunk of 256, with a
# carry: 256, 257 and 516 workgroups run the loop's body once, twice and three times, the last chunk partial.
BIG = (515 * T + 5, 256 * T, 256 * T + 1)
_BIG_RAYS = {}


def big_rays(r, n):
    """n rays on the `default` renderer r: the first half repeated_rays (heavy ties across workgroups), the second half
    seeded uniform origins over the box order_box() reports with seeded random directions of mixed sign.  Both halves
    are drawn once for the largest n and cut to size."""
    if not _BIG_RAYS:
        half = (max(BIG) + 1) // 2
        lo, scale = r.order_box()
        assert (scale > 0).all()
        hi = lo + np.float32(1 << oh.CB) / scale
        rng = np.random.default_rng(20240)
        uni = np.concatenate([rng.uniform(lo, hi, (half, 3)), rng.normal(size=(half, 3))], axis=1).astype(np.float32)
        assert all((uni[:, 3 + a] < 0).any() and (uni[:, 3 + a] > 0).any() for a in range(3))
        _BIG_RAYS.update(rep=repeated_rays(half), uni=uni)
    return np.concatenate([_BIG_RAYS["rep"][:n // 2], _BIG_RAYS["uni"][:n - n // 2]])


def test_order_past_256_workgroups():
    """One renderer, the scratch reused downward and up again: 516, 256 and 257 workgroups.  Every one of the 256 digit
    values occurs in each of the four passes, so every row of the scan's table carries counts across its chunks."""
    r, s, cam = renderer("default")
    assert [-(-n // T) for n in BIG] == [516, 256, 257]
    for n in BIG:
        rays = big_rays(r, n)
        order, keys = check_sort(r, rays, ("big", n))
        for p in range(4):
            seen = np.bincount((keys >> np.uint32(8 * p)) & np.uint32(255), minlength=256)
            assert (seen > 0).all(), (n, p, np.flatnonzero(seen == 0).tolist())
        assert len(np.unique(keys[:n // 2])) < n // 64  # the first half's keys repeat heavily
    r.close()


def test_paths_order_past_256_workgroups():
    """rfx_paths_order at the same scale: 256 T + 100 paths begun without a draw, an index array of 256 T + 200 slots of
    which 100 name no path -- the stable order of the restated keys, the 100 dead entries last, in index order"""
    n, slots = 256 * T + 100, 256 * T + 200
    r, s, cam = renderer("default")
    rays = big_rays(r, n)
    rng = np.random.default_rng(77)
    index = np.concatenate([rng.permutation(n), n + 1000 * np.arange(99), [0xFFFFFFFF]]).astype(np.uint32)[rng.permutation(slots)]
    real = index < n
    assert (~real).sum() == 100 and -(-slots // T) == 257
    before = r.get_rng()
    p = r.paths(rays, draw=False)
    got = p.order(index)
    p.close()
    assert r.get_rng() == before
    k = np.full(slots, 0xFFFFFFFF, np.uint32)
    k[real] = oh.keys(rays[index[real]], *r.order_box())
    assert (k[real] != 0xFFFFFFFF).all()
    want = index[oh.order(k)]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert np.array_equal(got[-100:], index[~real])
    r.close()


@pytest.mark.parametrize("n", [65, T + 1, 3 * T + 5])
def test_order_of_special_inputs(n):
    """All rays identical: the identity (stability); two alternating rays: one's indices, then the other's; input
    already in key order: the identity where keys differ and index order where they do not; in reverse key order."""
    r, s, cam = renderer("default")
    rays = repeated_rays(n)
    same = np.repeat(rays[:1], n, axis=0)
    order, keys = check_sort(r, same, ("identical", n))
    assert np.array_equal(order, np.arange(n)) and len(set(keys.tolist())) == 1
    two = incoherent_rays("default")[[3, 4]]
    lo, scale = r.order_box()
    k2 = oh.keys(two, lo, scale)
    assert k2[0] != k2[1]
    alt = np.tile(two, ((n + 1) // 2, 1))[:n]
    order, _ = check_sort(r, alt, ("alternating", n))
    first = 0 if k2[0] < k2[1] else 1
    assert np.array_equal(order, np.concatenate([np.arange(first, n, 2), np.arange(1 - first, n, 2)]))
    by_key = oh.order(oh.keys(rays, lo, scale))
    order, keys = check_sort(r, rays[by_key], ("sorted", n))
    assert np.array_equal(order, np.arange(n)) and (np.diff(keys.astype(np.int64)) >= 0).all()
    order, keys = check_sort(r, rays[by_key[::-1]], ("reversed", n))
    assert (np.diff(keys.astype(np.int64)) <= 0).all()
    r.close()


def test_order_optional_keys_and_sentinels():
    """d_keys NULL: the keys array stays as it was; given: every key is written; 64 sentinel words either side of the
    order and of the keys stay as they were."""
    import torch
    L = _lib.load()
    r, s, cam = renderer("default")
    for n in (357, T + 1):
        rays = repeated_rays(n)
        d_rays = dev(rays)
        want = oh.order(oh.keys(rays, *r.order_box()))
        for with_keys in (False, True):
            o = torch.full((PAD + n + PAD,), SENT, dtype=torch.int32, device="cuda")
            k = torch.full((PAD + n + PAD,), SENT, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
            _lib.check(L.rfx_rays_order(r._h, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(o.data_ptr() + 4 * PAD),
                                        C.c_void_p(k.data_ptr() + 4 * PAD) if with_keys else None, None))
            r.synchronize()
            o, k = u32(o), u32(k)
            assert (o[:PAD] == SENT).all() and (o[PAD + n:] == SENT).all(), (n, with_keys)
            assert np.array_equal(o[PAD:PAD + n], want), (n, with_keys)
            assert (k[:PAD] == SENT).all() and (k[PAD + n:] == SENT).all(), (n, with_keys)
            if with_keys:
                assert np.array_equal(k[PAD:PAD + n], oh.keys(rays, *r.order_box()))
            else:
                assert (k == SENT).all()
    r.close()


# ------------------------------------------------------------------ 3. the ordered trace
def trace(r, rays, order=None, depth=DEPTH, argb=True):
    """Renderer.trace_rays' device form on a side stream: (colours, ARGB words or None) as numpy."""
    def run():
        o = order if order is None or isinstance(order, str) else dev(np.asarray(order, np.uint32))
        return r.trace_rays(dev(rays), depth, argb=argb, order=o)
    out = side_stream(run)
    r.synchronize()  # (the pre-pass's error word)
    if argb:
        return out[0].cpu().numpy(), u32(out[1])
    return out.cpu().numpy(), None


def assert_colours(got, want, tag):
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (tag, bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


# (scene, tri_accel): between them every CFG bit the batch launcher can produce -- small with one light, planes, more
# than 32 lights, a large scene, a triangle tree
TRACE_SCENES = [("default", None), ("planes", None), ("lights40", None), ("stress4096", None), ("mesh40x32", 1)]


@pytest.mark.parametrize("name,tri_accel", TRACE_SCENES)
def test_ordered_trace_equals_the_per_ray_oracle(name, tri_accel):
    """357 incoherent rays under four orders -- the library's own, the identity, the reverse, a fixed random
    permutation -- give the CPU oracle's colours and ARGB words, and leave the sphere stream where the oracle's (and
    the unordered call's) stands."""
    rays = incoherent_rays(name)
    want, end, _ = incoherent_oracle(name)
    words = orc.argb_of(want)
    r, s, cam = renderer(name, tri_accel)
    if name == "mesh40x32":
        assert r.accel_info().tri_nodes > 0
    r.set_rng(SEED, 77)
    rgb, _ = trace(r, rays, argb=False)
    assert_colours(rgb, want, (name, "unordered"))
    assert r.get_rng() == (end, 77)
    own = device_order(r, rays)
    assert np.array_equal(np.sort(own), np.arange(NRAYS))
    for tag, order in (("coherent", "coherent"), ("own", own), ("identity", np.arange(NRAYS)),
                       ("reverse", np.arange(NRAYS)[::-1]), ("random", fixed_permutation(NRAYS))):
        r.set_rng(SEED, 77)
        rgb, argb = trace(r, rays, order)
        assert_colours(rgb, want, (name, tag))
        assert np.array_equal(argb, words), (name, tag)
        assert r.get_rng() == (end, 77), (name, tag)
    # d_argb NULL, and numpy in, numpy out
    r.set_rng(SEED, 77)
    rgb, _ = trace(r, rays, own, argb=False)
    assert_colours(rgb, want, (name, "no argb"))
    r.set_rng(SEED, 77)
    h_rgb, h_argb = r.trace_rays(rays, DEPTH, argb=True, order="coherent")
    assert_colours(h_rgb, want, (name, "host"))
    assert np.array_equal(h_argb, words) and r.get_rng() == (end, 77)
    r.close()


def test_ordered_trace_prefixes_and_the_frame_after():
    """Batches of 1, 63, 64 and 65 rays, in the library's order and reversed, are prefixes of the 357-ray result; a
    golden frame rendered after ordered batches is still its golden."""
    from reflaxman_amd.render import make_frame
    name = "default"
    rays = incoherent_rays(name)
    want = incoherent_oracle(name)[0]
    r, s, cam = renderer(name)
    for n in (1, 63, 64, 65):
        for order in ("coherent", np.arange(n)[::-1]):
            r.set_rng(SEED, 77)
            rgb, argb = trace(r, rays[:n], order)
            assert_colours(rgb, want[:n], (n, str(order)[:8]))
            assert np.array_equal(argb, orc.argb_of(want[:n]))
            assert r.get_rng()[0] == orc.rand_dirs(SEED, n)[1]
    key = "render_default_160x120_d4"
    c = manifest()["cases"][key]
    g = np.load(os.path.join(GOLDEN, key + ".npz"))
    r.set_rng(c["sphere_seed"], 0)
    img = np.zeros((c["H"], c["W"], 3), np.float32)
    f = make_frame(cam, c["W"], c["H"], c["depth"], 1)
    _lib.check(_lib.load().rfx_render_frame_host(r._h, C.byref(f), _lib.fptr(img), None, None))
    assert img.tobytes() == g["rgb"].tobytes()
    r.close()


# ------------------------------------------------------------------ 4. the ordered queries
# the scenes only these tests use take the rays of the scene they grew from
RAYS_OF = {"soup300_degenerate": "soup300", "mesh100_plane": "mesh100"}
# test_gpu_hits.py's list: (scene, tri_accel, the triangle tree the case is meant to run with: None = whatever it gives)
INCOHERENT = [("default", None, None), ("planes", None, None), ("synth16_sky", None, None), ("stress4096", None, None),
              ("planes300", None, None), ("mesh100", None, None), ("mesh40x32", None, None), ("soup300", None, None),
              ("mesh100", -1, False), ("mesh100", 1, True), ("mesh40x32", -1, True), ("mesh40x32", 2, True),
              ("soup300_degenerate", 1, True), ("mesh100_plane", 1, True)]


def hits(r, rays, order, **kw):
    out = side_stream(lambda: r.query_hits(dev(rays), order=order if isinstance(order, str) else dev(order), **kw))
    return {k: v.cpu().numpy() for k, v in out.items()}


def shadow(r, rays, order, skip=None):
    out = side_stream(lambda: r.occluded(dev(rays), None if skip is None else dev(np.asarray(skip, np.int32)),
                                         order=order if isinstance(order, str) else dev(order)))
    return out.cpu().numpy()


def assert_planes(got, want, tag):
    for k in got:
        bad = same_bits(got[k], want[k])
        assert bad.size == 0, (tag, k, bad[:8].tolist(), got[k][bad[:2]].tolist(), want[k][bad[:2]].tolist())


@pytest.mark.parametrize("name,tri_accel,tree", INCOHERENT)
def test_ordered_queries_equal_the_composed_reference(name, tri_accel, tree):
    """All six planes and the any-hit -- nothing left out, and each ray leaving out its own winner -- under the
    library's order and under a fixed random permutation."""
    rays = incoherent_rays(RAYS_OF.get(name, name))
    want, tab = compose(desc_of(name), rays, key=("incoherent", name))
    r, s, cam = renderer(name, tri_accel)
    if tree is not None:
        assert (r.accel_info().tri_nodes > 0) == tree, (name, tri_accel)
    for tag, order in (("coherent", "coherent"), ("random", fixed_permutation(NRAYS))):
        got = hits(r, rays, order)
        assert sorted(got) == sorted(PLANES)
        assert_planes(got, want, (name, tri_accel, tag))
        occ = shadow(r, rays, order)
        assert np.array_equal(occ, any_hit(tab)), (name, tag, np.flatnonzero(occ != any_hit(tab))[:8].tolist())
        own = shadow(r, rays, order, want["object"])
        ref = any_hit(tab, want["object"])
        assert np.array_equal(own, ref), (name, tag, np.flatnonzero(own != ref)[:8].tolist())
    r.close()


def test_ordered_queries_planes_alone_sentinels_and_splitting():
    """Each plane requested alone; 64 sentinel words either side of every buffer stay, an unrequested buffer stays
    wholly as it was; with the launch limit at one wave the slots run as six launches and no word changes; numpy in,
    numpy out."""
    import torch
    L = _lib.load()
    name = "planes300"
    rays = incoherent_rays(name)
    want, tab = compose(desc_of(name), rays, key=("incoherent", name))
    r, s, cam = renderer(name)
    order = device_order(r, rays)
    for k in PLANES:
        assert_planes(hits(r, rays, order, want=(k,)), {k: want[k]}, (name, "alone", k))
    d_rays, d_order = dev(rays), dev(order)
    words = {k: NRAYS * (1 if k in ("object", "distance") else 3) for k in PLANES}
    for limit, asked in ((0, PLANES), (64, PLANES), (0, ("object", "normal")), (1, ("distance", "colour"))):
        r.set_launch_traces(limit)
        buf = {k: torch.full((PAD + words[k] + PAD,), SENT, dtype=torch.int32, device="cuda") for k in PLANES}
        torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
        hp = _lib.HitPlanes()
        for k in asked:
            setattr(hp, k, buf[k].data_ptr() + 4 * PAD)
        _lib.check(L.rfx_query_hits_ordered(r._h, C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_order.data_ptr()), NRAYS,
                                            C.byref(hp), None))
        r.synchronize()
        for k in PLANES:
            b = buf[k].cpu().numpy()
            if k not in asked:
                assert (b == SENT).all(), (k, limit, asked)
                continue
            assert (b[:PAD] == SENT).all() and (b[PAD + words[k]:] == SENT).all(), (k, limit)
            got = b[PAD:PAD + words[k]].view(want[k].dtype).reshape(want[k].shape)
            assert same_bits(got, want[k]).size == 0, (k, limit, asked)
    # (the launch limit is still one wave)
    assert np.array_equal(shadow(r, rays, order, want["object"]), any_hit(tab, want["object"]))
    assert_planes(r.query_hits(rays, order="coherent"), want, (name, "host"))
    assert np.array_equal(r.occluded(rays, want["object"], order=order), any_hit(tab, want["object"]))
    r.close()


def test_order_and_ordered_queries_leave_the_renderer_state_alone():
    """The random streams read the same before and after an order call and ordered queries; the golden frame rendered
    after them is the golden frame; a rewind after "frame, order, ordered query" succeeds."""
    from reflaxman_amd.render import Render, build_scene
    key = "render_default_160x120_d4"
    c = manifest()["cases"][key]
    g = np.load(os.path.join(GOLDEN, key + ".npz"))
    W, H, depth = c["W"], c["H"], c["depth"]
    rays = incoherent_rays("default")
    want, tab = compose(desc_of("default"), rays, key=("incoherent", "default"))
    R = Render(sphere_seed=c["sphere_seed"], jitter_seed=0, load_default_scene=False)
    R.scene, R.camera = build_scene(scene("default"))
    R.setImageSize(W, H)
    r = R._r
    r.set_scene(R.scene)
    order = device_order(r, rays)
    assert_planes(hits(r, rays, order), want, "before")
    assert np.array_equal(shadow(r, rays, order), any_hit(tab))
    assert r.get_rng() == (c["sphere_seed"], 0)
    R.renderBegin(depth, 1, False)
    while R.renderNext(W * H):
        pass
    R.synchronize()
    assert R.image.tobytes() == g["rgb"].tobytes()
    after = r.get_rng()
    order = device_order(r, rays)
    assert_planes(hits(r, rays, order), want, "after the frame")
    assert np.array_equal(shadow(r, rays, "coherent", want["object"]), any_hit(tab, want["object"]))
    assert r.get_rng() == after
    assert _lib.load().rfx_frame_rng_rewind(r._h) == 0
    assert r.get_rng() == (c["sphere_seed"], 0)
    R.close()


# ------------------------------------------------------------------ 5. limits and errors
def test_limits_and_errors():
    import torch
    from reflaxman_amd.render import Renderer
    L = _lib.load()
    n = 128
    rays_h = incoherent_rays("default")[:n]
    rays = dev(rays_h)
    order = dev(np.arange(n, dtype=np.uint32))
    rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    obj = torch.zeros(n, dtype=torch.int32, device="cuda")
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
    p = lambda t: C.c_void_p(t.data_ptr())
    hp, none = _lib.HitPlanes(object=obj.data_ptr()), _lib.HitPlanes()
    bare = Renderer(sphere_seed=SEED)  # no scene
    assert L.rfx_rays_order(bare._h, p(rays), n, p(out), None, None) == RFX_ERR_STATE
    assert L.rfx_trace_rays_ordered(bare._h, p(rays), p(order), n, DEPTH, p(rgb), None, None) == RFX_ERR_STATE
    assert L.rfx_query_hits_ordered(bare._h, p(rays), p(order), n, C.byref(hp), None) == RFX_ERR_STATE
    assert L.rfx_query_occluded_ordered(bare._h, p(rays), None, p(order), n, p(occ), None) == RFX_ERR_STATE
    lo = np.zeros(3, np.float32)
    assert L.rfx_renderer_order_box(bare._h, _lib.fptr(lo), _lib.fptr(lo)) == RFX_ERR_STATE
    bare.close()
    r, s, cam = renderer("default")
    assert L.rfx_rays_order(r._h, p(rays), 0, p(out), None, None) == RFX_ERR_ARG
    assert L.rfx_rays_order(r._h, p(rays), 2 ** 31, p(out), None, None) == RFX_ERR_ARG
    assert L.rfx_rays_order(r._h, None, n, p(out), None, None) == RFX_ERR_ARG
    assert L.rfx_rays_order(r._h, p(rays), n, None, None, None) == RFX_ERR_ARG
    host = np.zeros(n, np.uint32)
    assert L.rfx_rays_order_host(r._h, None, n, _lib.u32ptr(host), None) == RFX_ERR_ARG
    assert L.rfx_rays_order_host(r._h, _lib.fptr(rays_h), n, None, None) == RFX_ERR_ARG
    assert L.rfx_rays_order_host(r._h, _lib.fptr(rays_h), 0, _lib.u32ptr(host), None) == RFX_ERR_ARG
    assert L.rfx_trace_rays_ordered(r._h, p(rays), p(order), 0, DEPTH, p(rgb), None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays_ordered(r._h, None, p(order), n, DEPTH, p(rgb), None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays_ordered(r._h, p(rays), None, n, DEPTH, p(rgb), None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays_ordered(r._h, p(rays), p(order), n, DEPTH, None, None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays_ordered(r._h, p(rays), p(order), n, 0, p(rgb), None, None) == RFX_ERR_ARG
    assert L.rfx_query_hits_ordered(r._h, p(rays), p(order), 0, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits_ordered(r._h, None, p(order), n, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits_ordered(r._h, p(rays), None, n, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits_ordered(r._h, p(rays), p(order), n, None, None) == RFX_ERR_ARG
    assert L.rfx_query_hits_ordered(r._h, p(rays), p(order), n, C.byref(none), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_ordered(r._h, p(rays), None, p(order), 0, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_ordered(r._h, None, None, p(order), n, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_ordered(r._h, p(rays), None, None, n, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_ordered(r._h, p(rays), None, p(order), n, None, None) == RFX_ERR_ARG
    # an ordered trace above the launch limit is refused before anything moves
    r.set_launch_traces(n - 1)
    assert L.rfx_trace_rays_ordered(r._h, p(rays), p(order), n, DEPTH, p(rgb), None, None) == RFX_ERR_ARG
    r.synchronize()
    assert r.get_rng() == (SEED, 77)
    assert (rgb.cpu().numpy() == 7.0).all()
    r.set_launch_traces(n)
    assert L.rfx_trace_rays_ordered(r._h, p(rays), p(order), n, DEPTH, p(rgb), None, None) == 0
    r.synchronize()
    assert_colours(rgb.cpu().numpy(), incoherent_oracle("default")[0][:n], "at the limit")
    assert r.get_rng()[0] == orc.rand_dirs(SEED, n)[1]
    # the Python layer: an order goes with no raster and no counters, and names every ray once
    with pytest.raises(ValueError):
        r.trace_rays(rays, DEPTH, raster_width=8, order="coherent")
    with pytest.raises(ValueError):
        r.trace_rays(rays, DEPTH, counters=torch.zeros(_lib.RFX_NCOUNTERS, dtype=torch.int64, device="cuda"), order=order)
    with pytest.raises(ValueError):
        r.query_hits(rays, raster_width=8, order=order)
    with pytest.raises(ValueError):
        r.occluded(rays, raster_width=8, order="coherent")
    with pytest.raises(ValueError):
        r.query_hits(rays, order=order[:n - 1])
    with pytest.raises(ValueError):
        r.trace_rays(rays_h, DEPTH, order="sorted")
    r.close()


# ------------------------------------------------------------------ 6. the index guard
def test_an_index_outside_the_batch_is_a_dead_lane():
    """No fault is possible here: every ray-indexed array is 64 entries longer than n, sentinels in the padding.  The
    order holds n and n + 5 where two real indices should stand: the padding and the two absent rays' outputs keep
    their sentinels, and every other ray is exact."""
    import torch
    L = _lib.load()
    name = "default"
    n, extra = 200, 64
    rays = incoherent_rays(name)[:n]
    want, tab = compose(desc_of(name), incoherent_rays(name), key=("incoherent", name))
    colours = incoherent_oracle(name)[0][:n]
    r, s, cam = renderer(name)
    order = device_order(r, rays).copy()
    absent = [int(order[17]), int(order[130])]
    order[17], order[130] = n, n + 5
    present = np.setdiff1d(np.arange(n), absent)
    # the padding's rays are real rays, its skips real objects: were a dead lane to run, its output would change
    padded = np.concatenate([rays, incoherent_rays(name)[n:n + extra]])
    d_rays, d_order = dev(padded), dev(order)
    d_skip = dev(np.concatenate([want["object"][:n], np.zeros(extra, np.int32)]).astype(np.int32))
    full = lambda words, dtype=torch.int32: torch.full(((n + extra) * words,), SENT, dtype=dtype, device="cuda")
    buf = {k: full(1 if k in ("object", "distance") else 3) for k in PLANES}
    d_occ = torch.full((n + extra,), 0x5A, dtype=torch.uint8, device="cuda")
    d_rgb, d_argb = full(3), full(1)
    torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = _lib.HitPlanes()
    for k in PLANES:
        setattr(hp, k, buf[k].data_ptr())
    _lib.check(L.rfx_query_hits_ordered(r._h, p(d_rays), p(d_order), n, C.byref(hp), None))
    _lib.check(L.rfx_query_occluded_ordered(r._h, p(d_rays), p(d_skip), p(d_order), n, p(d_occ), None))
    _lib.check(L.rfx_trace_rays_ordered(r._h, p(d_rays), p(d_order), n, DEPTH, p(d_rgb), p(d_argb), None))
    r.synchronize()

    def check(words, ref, tag):
        w = words.reshape(n + extra, -1)
        assert (w[n:] == SENT).all() and (w[absent] == SENT).all(), tag
        got = np.ascontiguousarray(w[present]).view(ref.dtype).reshape((len(present),) + ref.shape[1:])
        assert same_bits(got, ref[present]).size == 0, tag

    for k in PLANES:
        check(buf[k].cpu().numpy(), want[k][:n], k)
    occ = d_occ.cpu().numpy()
    assert (occ[n:] == 0x5A).all() and (occ[absent] == 0x5A).all()
    assert np.array_equal(occ[present], any_hit(tab, want["object"])[:n][present])
    check(d_rgb.cpu().numpy(), colours, "rgb")
    check(d_argb.cpu().numpy(), orc.argb_of(colours).astype(np.uint32).reshape(-1, 1), "argb")
    assert r.get_rng()[0] == orc.rand_dirs(SEED, n)[1]  # the stream moves by n draws whatever the order names
    r.close()
