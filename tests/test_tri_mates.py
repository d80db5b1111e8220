"""Coplanar mates (rfx_scene.cpp tri_mate_leaders, rfx.h rfx_scene_tri_mates): the host's grouping rule, bit for bit,
and a float32 replay of the z stage of Triangle::trace (rfx_intersect.h tri_z / tri_zt) showing that every member of a group
the host reports gives the same plane crossing for the same ray.  No GPU: the scene builder is host code."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from reflaxman_amd import scenes
from reflaxman_amd.render import build_scene
from reflaxman_amd.scenes import DIELECTRIC, METAL

VERY_SMALL = np.float32(1.0842021724855044e-19)
DELTA = np.float32(0.0001)
WHITE = (1.0, 1.0, 1.0)


def scene_of(tris, name="mates"):
    s = scenes._base(name)
    for k, (a, b, c) in enumerate(tris):
        s.add_triangle(a, b, c, METAL if k % 2 else DIELECTRIC, WHITE, 0.5)
    return s


def mates(desc, on=True):
    """(leader, rows): rows[t] = v0 x y z, a31 a32 a33 as the host holds them."""
    s, _ = build_scene(desc)
    if not on:
        s.set_tri_mates(False)
    return s.tri_mates(plane=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rule_holds(rows, a, b) -> bool:
    """The mate rule for triangles a and b, restated on the bits."""
    ra, rb = rows[a], rows[b]
    if not (np.isfinite(ra).all() and np.isfinite(rb).all()):
        return False
    if not np.array_equal(bits(ra[3:]), bits(rb[3:])):
        return False
    return all(bits(ra[i]) == bits(rb[i]) or ra[3 + i] == 0.0 for i in range(3))


def check_partition(leader, rows):
    """What the host reports is the rule's partition: a leader is the lowest index of its group, members satisfy the
    rule with their leader, and two triangles of different groups do not."""
    n = len(leader)
    for t in range(n):
        l = int(leader[t])
        assert 0 <= l <= t and leader[l] == l
        if l != t:
            assert rule_holds(rows, l, t), (l, t, rows[l], rows[t])
    heads = [t for t in range(n) if leader[t] == t]
    for i, a in enumerate(heads):
        for b in heads[i + 1:]:
            assert not rule_holds(rows, a, b), (a, b)


def quad(p, e1, e2, flip=False):
    """Two triangles (a, b, c), (b, d, c) of a = p, b = p + e1, c = p + e2, d = p + e1 + e2, the ground quad's pattern;
    flip: (a, c, b), (d, b, c), the normal the other way (in a vertex order that gives both triangles' third rows the
    same zero signs: the rule compares bits, and (0, 1, 0) and (-0, 1, 0) are different rows)."""
    p, e1, e2 = (np.array(v, np.float64) for v in (p, e1, e2))
    a, b, c, d = p, p + e1, p + e2, p + e1 + e2
    t = ((a, c, b), (d, b, c)) if flip else ((a, b, c), (b, d, c))
    return [tuple(tuple(float(x) for x in q) for q in tr) for tr in t]


# ------------------------------------------------------------------ the rule on the host
def test_leaders_of_the_stock_scenes():
    assert mates(scenes.get_scene("synth16"))[0].tolist() == [0, 0, 2, 2]
    assert mates(scenes.get_scene("default"))[0].tolist() == [0, 0]
    assert mates(scenes.get_scene("synth16"), on=False)[0].tolist() == [0, 1, 2, 3]
    assert mates(scenes.get_scene("default"), on=False)[0].tolist() == [0, 1]
    for name in ("synth16", "default"):
        check_partition(*mates(scenes.get_scene(name)))


def test_rotated_quad_and_tilted_fan_obey_the_rule():
    """Whatever the host decides for planes that are not axis-aligned satisfies the rule bit for bit."""
    c, s = np.cos(0.37), np.sin(0.37)
    tris = quad((0.3, 0.0, -0.2), (4 * c, 0.0, 4 * s), (-3 * s, 0.0, 3 * c))           # rotated about y, in y = 0
    tris += quad((1.0, 0.5, 2.0), (2 * c, 2 * s, 0.1), (-0.3, 0.2, 1.7))                 # rotated and tilted
    v0, v1, v2, v3 = (0.1, 0.2, 0.3), (2.1, 0.9, 0.4), (2.3, 1.4, 2.2), (0.2, 0.8, 2.5)  # a fan on a tilted plane
    v3 = tuple(np.array(v0) + 0.4 * (np.array(v1) - np.array(v0)) + 0.9 * (np.array(v2) - np.array(v0)))
    tris += [(v0, v1, v2), (v0, v2, v3)]
    leader, rows = mates(scene_of(tris))
    check_partition(leader, rows)


def test_near_misses_do_not_group():
    # the same quad at two heights: v0 differs on the axis that row 3 weighs
    tris = quad((0, 0, 0), (0, 0, 2), (2, 0, 0)) + quad((0, 1, 0), (0, 0, 2), (2, 0, 0))
    leader, rows = mates(scene_of(tris))
    assert leader.tolist() == [0, 0, 2, 2] and rows[0][4] != 0.0 and rows[0][1] != rows[2][1]
    check_partition(leader, rows)
    # one vertex moved ulp by ulp on a tilted plane: v0 stays, row 3 changes by single ulps
    base = ((0.0, 0.0, 0.0), (1.0, 0.3, 0.0), (0.0, 0.2, 1.0))
    tris = [base]
    y = np.float32(0.3)
    for _ in range(64):
        y = np.nextafter(y, np.float32(1.0))
        tris.append((base[0], (1.0, float(y), 0.0), base[2]))
    leader, rows = mates(scene_of(tris))
    check_partition(leader, rows)
    d = np.abs(bits(rows[:, 3:]).astype(np.int64) - bits(rows[0, 3:]).astype(np.int64)).sum(axis=1)
    one_ulp = np.flatnonzero(d == 1)
    assert one_ulp.size, d
    assert all(leader[t] != 0 for t in one_ulp)


def test_non_finite_records_do_not_group():
    inf, nan = float("inf"), float("nan")
    tris = []
    for v0 in ((inf, 0, 0), (0, -inf, 0), (0, 0, nan)):
        tris += [(v0, (1, 0, 0), (0, 0, 1))] * 2
    for v1 in ((nan, 0, 0), (1, inf, 0)):
        tris += [((0, 0, 0), v1, (0, 0, 1))] * 2
    leader, rows = mates(scene_of(tris))
    bad = ~np.isfinite(rows).all(axis=1)
    assert bad[:6].all()
    assert all(leader[t] == t for t in np.flatnonzero(bad))
    assert not any(bad[leader[t]] for t in range(len(leader)) if leader[t] != t)
    check_partition(leader, rows)


@functools.lru_cache(maxsize=None)
def constructed():
    """Axis-aligned quads on all three axes in both windings (six groups), unrelated triangles between them, and a
    third triangle in the first quad's plane added last: a three-member group whose members are not adjacent."""
    tris = []
    filler = [((5.0, 1.0 + k, 2.0), (6.5, 2.25 + k, 2.5), (5.25, 1.5 + k, 4.0)) for k in range(6)]
    quads = [((-3, 0.5, -2), (0, 0, 4), (6, 0, 0)), ((-3, 2.5, -2), (0, 0, 4), (6, 0, 0)),     # y planes
             ((-4, 0, -2), (0, 3, 0), (0, 0, 4)), ((7, 0, -2), (0, 3, 0), (0, 0, 4)),          # x planes
             ((-3, 0, -5), (6, 0, 0), (0, 3, 0)), ((-3, 0, 6), (6, 0, 0), (0, 3, 0))]          # z planes
    for k, (p, e1, e2) in enumerate(quads):
        tris += quad(p, e1, e2, flip=bool(k & 1))
        tris.append(filler[k])
    tris.append(((10.0, 0.5, 10.0), (10.0, 0.5, 12.0), (12.0, 0.5, 10.0)))  # coplanar with quad 0, far from it
    return scene_of(tris, "mates_axes")


def test_non_adjacent_members_form_one_group():
    leader, rows = mates(constructed())
    check_partition(leader, rows)
    assert leader[0] == 0 and leader[1] == 0 and leader[-1] == 0 and leader[2] == 2  # the filler between them is not
    groups = group_lists(leader)
    assert len(groups) >= 6
    assert any(len(g) == 3 for g in groups)
    assert any(max(np.diff(g)) > 1 for g in groups)


def group_lists(leader):
    out = {}
    for t, l in enumerate(leader.tolist()):
        out.setdefault(l, []).append(t)
    return [g for g in out.values() if len(g) > 1]


# ------------------------------------------------------------------ the float32 replay of the z stage
def z_stage(row, o, ray, best_sq):
    """tri_z and tri_zt for one triangle's (v0, row 3) and arrays of origins and rays, in float32 with the reference's
    operation order (every product and sum rounded on its own: numpy has no FMA contraction).  Returns the values the
    stages derive and the decisions they take."""
    f = np.float32
    v0x, v0y, v0z, a31, a32, a33 = (f(x) for x in row)
    with np.errstate(all="ignore"):
        dx, dy, dz = o[:, 0] - v0x, o[:, 1] - v0y, o[:, 2] - v0z
        aoz = dx * a31 + dy * a32 + dz * a33
        arz = ray[:, 0] * a31 + ray[:, 1] * a32 + ray[:, 2] * a33
        far = np.abs(arz) > VERY_SMALL
        nz = -aoz
        same = ((nz > 0) & (arz > 0)) | ((nz < 0) & (arz < 0))
        a2 = f(2.0) * (ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1] + ray[:, 2] * ray[:, 2])
        n2a, r2 = nz * nz * a2, arz * arz
        near = n2a < (f(2.0) * (DELTA * DELTA)) * r2 * f(0.99997)
        beyond = n2a > best_sq * r2 * f(2.0000305)
        t = nz / arz
        tpos = t > VERY_SMALL
        rt = ray * t[:, None]
        sq = rt[:, 0] * rt[:, 0] + rt[:, 1] * rt[:, 1] + rt[:, 2] * rt[:, 2]
        keep = sq > DELTA * DELTA
    return {"aoz": aoz, "arz": arz, "n2a": n2a, "r2": r2, "t": t, "sq": sq}, \
           {"far": far, "same": same, "near": near, "beyond": beyond, "tpos": tpos, "keep": keep}


@functools.lru_cache(maxsize=None)
def random_pairs():
    """10^6 origin / ray pairs: origins log-uniform in magnitude from 2^-20 to 2^30 with either sign, rays of every
    direction with lengths from 2^-10 to 2^10; a best distance from 0 to +inf.  Read-only."""
    rng = np.random.default_rng(20261019)
    n = 1_000_000
    o = (np.exp2(rng.uniform(-20, 30, (n, 3))) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    ray = (rng.normal(size=(n, 3)) * np.exp2(rng.uniform(-10, 10, (n, 1)))).astype(np.float32)
    best = np.exp2(rng.uniform(-30, 40, n)).astype(np.float32)
    best[::7] = np.inf
    for a in (o, ray, best):
        a.setflags(write=False)
    return o, ray, best


def edge_pairs(rows, members):
    """The listed edge cases for one group: origins exactly on the plane, at every member's v0, rays parallel to the
    plane, origins with an infinite or NaN component, coordinates up to 2^30."""
    f = np.float32
    row = rows[members[0]]
    n = row[3:].astype(np.float64)
    axis = int(np.argmax(np.abs(n)))
    others = [i for i in range(3) if i != axis]
    rays = [(0.3, -0.7, 0.5), (-1.0, 0.25, 2.0), (1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)]
    par = np.zeros(3)
    par[others[0]], par[others[1]] = 0.8, -0.6   # in the plane when it is axis-aligned
    u = np.cross(n, [0.3, 0.5, 0.7])             # in any plane, up to rounding
    rays += [tuple(par), tuple(u), tuple(-u)]
    origins = []
    for m in members:
        v0 = rows[m][:3].astype(np.float64)
        origins.append(v0)                                                    # at a member's v0
        for d in ((1.5, -2.25), (-1024.0, 3.0), (2.0 ** 30, -(2.0 ** 30))):   # on the plane (axis-aligned: exactly)
            p = v0.copy()
            p[others[0]] += d[0]
            p[others[1]] += d[1]
            origins.append(p)
        origins.append(v0 + u * 3.0)
    origins += [(2.0 ** 30, 2.0 ** 30, -(2.0 ** 30)), (-(2.0 ** 30), 1.0, 2.0 ** 29), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)]
    for i in range(3):
        for bad in (np.inf, -np.inf, np.nan):
            p = np.array([0.5, 0.25, -0.75])
            p[i] = bad
            origins.append(p)
    origins.append((np.inf, -np.inf, np.nan))
    o = np.array([p for p in origins for _ in rays], f)
    ray = np.array([r for _ in origins for r in rays], f)
    best = np.full(len(o), np.inf, f)
    best[::2] = f(50.0)
    return o, ray, best


def same_or_nan_together(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def replay(desc):
    """Every group of the scene: each member's z stage against its leader's; returns the groups checked."""
    leader, rows = mates(desc)
    check_partition(leader, rows)
    groups = group_lists(leader)
    for g in groups:
        for o, ray, best in (random_pairs(), edge_pairs(rows, g)):
            want_v, want_d = z_stage(rows[g[0]], o, ray, best)
            for m in g[1:]:
                got_v, got_d = z_stage(rows[m], o, ray, best)
                for k in want_v:
                    assert same_or_nan_together(want_v[k], got_v[k]), (desc.name, g, m, k)
                for k in want_d:
                    assert np.array_equal(want_d[k], got_d[k]), (desc.name, g, m, k)
    return groups


@pytest.mark.parametrize("name", ["synth16", "default", "soup300_degenerate", "mesh100"])
def test_replay_of_the_stock_scenes(name):
    desc = scenes.degenerate_soup_scene() if name == "soup300_degenerate" else scenes.get_scene(name)
    groups = replay(desc)
    if name in ("synth16", "default", "soup300_degenerate"):  # the ground quad at least
        assert groups


def test_replay_of_the_constructed_scene():
    groups = replay(constructed())
    assert len(groups) >= 6 and any(len(g) == 3 for g in groups) and any(max(np.diff(g)) > 1 for g in groups)


def test_the_replay_can_fail():
    """The comparison is live: two parallel planes differ in aoz, and the replay sees it."""
    leader, rows = mates(scene_of(quad((0, 0, 0), (0, 0, 2), (2, 0, 0)) + quad((0, 1, 0), (0, 0, 2), (2, 0, 0))))
    o, ray, best = edge_pairs(rows, [0, 2])
    a, _ = z_stage(rows[0], o, ray, best)
    b, _ = z_stage(rows[2], o, ray, best)
    assert not same_or_nan_together(a["aoz"], b["aoz"])


# ------------------------------------------------------------------ the host code under the sanitizers
def test_host_code_under_sanitizers(tmp_path):
    """rfx_scene.cpp with a stand-alone checker (tests/native/tri_mates_check.cpp) by plain g++ under ASan and UBSan:
    no HIP, nothing loaded into Python."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "reflaxman_amd", "csrc")
    exe = str(tmp_path / "tri_mates_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + csrc, os.path.join(csrc, "rfx_scene.cpp"),
                    os.path.join(root, "tests", "native", "tri_mates_check.cpp"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
