"""Far lights (rfx_scene.cpp far_light_terms / far_light_scene, rfx.h rfx_scene_far_light): the host's rule on the stock
scenes and on lights that must not qualify, a float32 replay of `light - hit == light` inside the bound the host
reports, the record's constants against the general expressions of Scene::trace restated in numpy float32, and the
shadow rays' cone.  No GPU: the scene builder is host code."""
from __future__ import annotations

import numpy as np
import pytest

from reflaxman_amd import scenes
from reflaxman_amd.render import build_scene
from reflaxman_amd.scenes import METAL

f32 = np.float32
VERY_SMALL = f32(1.0842021724855044e-19)
SUN = ((11.8e9, 4.26e9, 3.08e9), 3.48e8)
POW2 = ((2.0 ** 33, -3.0e10, 2.0 ** 33), 1.0e8)
GUARD = ((9.0e6, 1.1e7, 1.2e7), 3.0e5)
LIGHTS = {"sun": SUN, "pow2": POW2, "guard": GUARD}


def one_light_scene(origin, radius, extent=2.0):
    s = scenes._base("far")
    s.add_light(origin, radius, (1.0, 1.0, 1.0), 0.9)
    s.add_sphere((extent - 1.0, 0.0, 0.0), 1.0, METAL, (1.0, 1.0, 1.0), 0.5)
    s.add_triangle((-extent, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), METAL, (1.0, 1.0, 1.0), 0.5)
    return s


def far_light(desc, mode=None):
    """(chosen, {name: float32 term}) of the scene's first light."""
    s, _ = build_scene(desc)
    if mode is not None:
        s.set_far_lights(mode)
    chosen, t = s.far_light(0)
    return chosen, dict(zip(("dlen", "ndx", "ndy", "ndz", "spec_add", "near", "cone_cos", "cone_sin"), t))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def spacing_below(x):
    x = np.abs(f32(x))
    return x - np.nextafter(x, f32(0.0))


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("name", ["default", "synth16", "stress4096"])
def test_the_sun_is_far_on_the_stock_scenes(name):
    desc = scenes.get_scene(name)
    assert len(desc.lights) == 1
    o, r, _, _ = desc.lights[0]
    assert bits(o).tolist() == bits(SUN[0]).tolist() and f32(r) == f32(SUN[1])
    chosen, t = far_light(desc)
    assert chosen and t["near"] == 128.0
    assert [float(spacing_below(c)) for c in o] == [1024.0, 256.0, 256.0]
    assert not far_light(desc, 0)[0] and far_light(desc, 0)[1]["near"] == 128.0 and far_light(desc, 2)[0]


@pytest.mark.parametrize("origin,radius", [((0.0, 4.26e9, 3.08e9), 3.48e8), ((1e9, -0.0, 1e9), 1e7),
                                           ((1e9, 1e9, 1e9), 0.9e9), ((1e9, 1e9, 1e9), 2e9),
                                           ((np.inf, 1e9, 1e9), 1e7), ((1e9, np.nan, 1e9), 1e7),
                                           ((1e9, 1e9, 1e9), np.inf), ((1e9, 1e9, 1e9), np.nan)])
def test_lights_the_rule_refuses(origin, radius):
    for mode in (1, 2):
        chosen, t = far_light(one_light_scene(origin, radius), mode)
        assert not chosen and all(v == 0.0 for v in t.values())


def test_a_near_light_gets_too_small_a_bound():
    chosen, t = far_light(one_light_scene((5.0, 8.0, 3.0), 0.5))
    assert not chosen and 0.0 < t["near"] == spacing_below(3.0) / 2  # 8 is a power of two: its spacing below is 3's twice
    assert far_light(one_light_scene((5.0, 8.0, 3.0), 0.5), 2)[0]    # far by the rule: the forced mode takes it


def test_a_scene_wider_than_the_bound_is_not_chosen():
    assert far_light(one_light_scene(*SUN, extent=127.5))[0]
    assert not far_light(one_light_scene(*SUN, extent=128.0))[0]  # the compare is strict
    assert far_light(one_light_scene(*SUN, extent=128.0), 2)[0]
    two = one_light_scene(*SUN)
    two.add_light((1e9, 2e9, 3e9), 1e7, (1.0, 1.0, 1.0), 0.5)
    assert not far_light(two)[0] and not far_light(two, 2)[0]


def test_a_power_of_two_coordinate_uses_the_halved_spacing():
    chosen, t = far_light(one_light_scene(*POW2))
    assert chosen and t["near"] == 256.0  # 2^33: floats 1024 apart above it, 512 below
    assert spacing_below(2.0 ** 33) == 512.0 and np.nextafter(f32(2.0 ** 33), f32(np.inf)) - f32(2.0 ** 33) == 1024.0
    assert far_light(one_light_scene(*GUARD))[1]["near"] == 0.5


# ------------------------------------------------------------------ float32 replay: light - hit == light
@pytest.mark.parametrize("name", sorted(LIGHTS))
def test_light_minus_hit_is_the_light_inside_the_bound(name):
    origin, radius = LIGHTS[name]
    near = far_light(one_light_scene(origin, radius), 2)[1]["near"]
    L = np.asarray(origin, f32)
    rng = np.random.default_rng(20261020)
    inner = np.nextafter(near, f32(0.0))
    d = rng.uniform(-float(near), float(near), (1_000_000, 3)).astype(f32)
    d = np.clip(d, -inner, inner)  # the rounding to float32 may reach the bound itself
    edges = np.array([[sx * inner, sy * inner, sz * inner] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)], f32)
    tiny = np.array([[1e-30, -1e-30, 0.0], [-0.0, 0.0, -0.0]], f32)
    for pts in (d, edges, tiny):
        assert pts.dtype == f32 and np.all(np.abs(pts) < near)
        diff = L[None, :] - pts
        assert diff.dtype == f32 and np.array_equal(bits(diff), np.broadcast_to(bits(L), diff.shape))
    # at the bound itself a tie rounds to the even neighbour, which is the light only where its significand is even: the
    # sun's y is odd and moves, so the kernels' compare must be strict
    if name == "sun":
        at = np.array([[sx * near, sy * near, sz * near] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], f32)
        moved = bits(L[None, :] - at) != bits(L)[None, :]
        assert moved[:, 1].any() and not moved[:, 0].any()


# ------------------------------------------------------------------ the record's constants
def general_terms(origin, radius):
    """Scene.cpp:117-181 for dirToLight = L (rfx_bounce.h's general form) in float32, operation for operation."""
    x, y, z = (f32(c) for c in origin)
    r = f32(radius)
    sq = x * x + y * y + z * z
    dlen = np.sqrt(sq)
    assert sq > VERY_SMALL and dlen > VERY_SMALL
    ang = f32(1.0) - (r * r) / sq
    nd = (x / dlen, y / dlen, z / dlen)
    return {"dlen": dlen, "ndx": nd[0], "ndy": nd[1], "ndz": nd[2], "spec_add": f32(1.0) - np.sqrt(ang), "ang": ang}


def cone_terms(radius, dlen):
    """rfx_bundle.h make_bundle_ball's widening for a lane whose ray is the axis (ca = 1, sa = 0), in float32."""
    sb = min(f32(radius) / dlen * f32(1.001), f32(1.0))
    cb = np.sqrt(max(f32(1.0) - sb * sb, f32(0.0)))
    dev = max(f32(1.0) - cb, f32(0.0))
    cosa = f32(1.0) - dev - f32(4e-6)
    sina = np.sqrt(max(f32(1.0) - cosa * cosa, f32(0.0)) + f32(1e-7)) * f32(1.001)
    return sb, cosa, sina


@pytest.mark.parametrize("name", sorted(LIGHTS))
def test_the_record_holds_the_general_expressions_bits(name):
    origin, radius = LIGHTS[name]
    t = far_light(one_light_scene(origin, radius), 2)[1]
    want = general_terms(origin, radius)
    assert want["ang"] > 0 and all(type(v) is f32 for v in want.values())
    for k in ("dlen", "ndx", "ndy", "ndz", "spec_add"):
        assert bits(t[k]) == bits(want[k]), k
    sb, cosa, sina = cone_terms(radius, want["dlen"])
    assert sb < 0.5 and bits(t["cone_cos"]) == bits(cosa) and bits(t["cone_sin"]) == bits(sina)


@pytest.mark.parametrize("name", sorted(LIGHTS))
def test_the_cone_contains_the_shadow_rays(name):
    origin, radius = LIGHTS[name]
    t = far_light(one_light_scene(origin, radius), 2)[1]
    L, R = np.asarray(origin, f32), f32(radius)
    rng = np.random.default_rng(7)
    rd = rng.uniform(-1.0, 1.0, (400_000, 3)).astype(f32)
    rd = rd[(rd.astype(np.float64) ** 2).sum(1) <= 1.0][:100_000]
    unit = rd / np.sqrt((rd.astype(np.float64) ** 2).sum(1))[:, None]
    rd = np.concatenate([rd, unit.astype(f32)[:20_000]])  # and the ball's surface, where the angle is widest
    assert len(rd) == 120_000
    sray = L[None, :] + rd * R  # Scene.cpp:129 in float32
    assert sray.dtype == f32
    v = sray.astype(np.float64)
    axis = np.array([t["ndx"], t["ndy"], t["ndz"]], np.float64)
    cos = (v @ axis) / np.sqrt((v * v).sum(1)) / np.sqrt(axis @ axis)
    assert cos.min() > float(t["cone_cos"])
    # the widest ray is the ball's tangent: the cone is no wider than 1.1 times its angle plus the fixed widening
    beta = np.arcsin(float(R) / float(t["dlen"]))
    assert np.arccos(cos.min()) > 0.9 * beta
    assert np.arccos(float(t["cone_cos"])) < 1.1 * beta + np.sqrt(2 * 4e-6) + 1e-3
    assert float(t["cone_sin"]) >= np.sqrt(1.0 - float(t["cone_cos"]) ** 2)


# ------------------------------------------------------------------ the host code under the sanitizers
def test_host_code_under_sanitizers(tmp_path):
    """rfx_scene.cpp with a stand-alone checker (tests/native/far_light_check.cpp) by plain g++ under ASan and UBSan:
    no HIP, nothing loaded into Python."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "reflaxman_amd", "csrc")
    exe = str(tmp_path / "far_light_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + csrc, os.path.join(csrc, "rfx_scene.cpp"),
                    os.path.join(root, "tests", "native", "far_light_check.cpp"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
