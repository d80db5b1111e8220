"""Python mirror of the reference's Render / Scene / Camera / Material API.

Same names, argument meaning and error behaviour as the reference's C++
classes (src/common/Render.h:7-42, Scene.h:28-40, Camera.h:30-62,
Material.h:5-19, OmniLight.h, Color.h, Vector3.h, Texture.h), implemented over
the C-ABI of librfx.so (include/rfx.h).  Every trace runs in the HIP kernels;
there is no CPU path.

Drop-in semantics (Render.cpp:57-226):
  * ``setImageSize`` zero-fills the float framebuffer, resets the cursor and
    ``additiveCounter``;
  * ``renderBegin`` snapshots the camera and bumps/clears ``additiveCounter``;
  * ``renderNext(pixels)`` renders exactly the raster span the reference's
    cursor would cover -- on the GPU, one launch per call -- and returns
    ``inProgress``.  Chunked callers (Pulse.cpp:102-209) therefore get the
    reference's image for any chunk pattern;
  * ``renderAll`` keeps the reference's behaviour (renders ``imageHeight``
    *pixels*, Render.cpp:217-221);
  * ``imagePixel`` divides by ``additiveCounter`` when it is > 1, ``copyImage``
    does not (Render.cpp:82-114).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import DIELECTRIC, METAL, check, farr

DEFAULT_SPHERE_SEED = 1350490027  # glibc rand() #12: Vector3.cpp's stream in the survey's link order
DEFAULT_JITTER_SEED = 424238335   # glibc rand() #6:  Render.cpp's stream in the same link order


class Vector3:
    __slots__ = ("x", "y", "z")

    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = float(x), float(y), float(z)

    def __iter__(self):
        return iter((self.x, self.y, self.z))

    def __repr__(self):
        return f"Vector3({self.x}, {self.y}, {self.z})"


class Color:
    __slots__ = ("r", "g", "b")

    def __init__(self, r=0.0, g=0.0, b=0.0):
        self.r, self.g, self.b = float(r), float(g), float(b)

    def __iter__(self):
        return iter((self.r, self.g, self.b))

    def argb(self) -> int:
        """Color::argb (Color.cpp:114-117)."""
        out = (C.c_uint32 * 1)()
        _lib.load().rfx_argb_from_rgb(farr(self), 1, out)
        return int(out[0])

    def __repr__(self):
        return f"Color({self.r}, {self.g}, {self.b})"


class Material:
    """Material(type, color, reflectivity, transparency) -- Material.cpp:8-14 (clamping happens in the library)."""
    mtMetal, mtDielectric = METAL, DIELECTRIC

    def __init__(self, type=METAL, color: Color = Color(1, 1, 1), reflectivity=0.0, transparency=0.0):
        if type not in (METAL, DIELECTRIC):
            raise ValueError("Material type must be Material.mtMetal or Material.mtDielectric")
        self.type = type
        self.color = Color(*color)
        self.reflectivity = float(reflectivity)
        self.transparency = float(transparency)


class Camera:
    """Camera(eye, at, fov): the rendering-relevant part (Camera.cpp:24-56).  ``view`` is row-major _11.._33."""

    def __init__(self, eye=Vector3(), at=Vector3(0, 0, 1), fov=1.0):
        self.eye = Vector3(*eye)
        self.fov = float(fov)
        view = (C.c_float * 9)()
        _lib.load().rfx_camera_view(farr(self.eye), farr(Vector3(*at)), view)
        self.view = [float(v) for v in view]


class Texture:
    """Handle of a scene texture (Scene::addTexture's returned Texture*)."""

    def __init__(self, scene: "Scene", index: int, loaded: bool):
        self.scene, self.index, self.loaded = scene, index, loaded


class Triangle:
    """Handle of a scene triangle (Scene::addTriangle's returned Triangle*)."""

    def __init__(self, scene: "Scene", obj: int):
        self.scene, self.obj = scene, obj

    def setTexture(self, texture: Optional[Texture], u1, v1, u2, v2, u3, v3):  # Triangle.cpp:110-120
        if texture is None:
            raise ValueError("setTexture needs a texture from Scene.addTexture")
        check(_lib.load().rfx_triangle_set_texture(self.scene._h, self.obj, texture.index, farr((u1, v1, u2, v2, u3, v3))),
              "Triangle.setTexture")
        self.scene._version += 1


class Sphere:
    def __init__(self, scene: "Scene", obj: int):
        self.scene, self.obj = scene, obj


class Plane:
    """Handle of a scene plane (Scene.addPlane, the extension of Scene::add* to Plane.h's primitive)."""

    def __init__(self, scene: "Scene", obj: int):
        self.scene, self.obj = scene, obj


class OmniLight:
    def __init__(self, scene: "Scene", index: int):
        self.scene, self.index = scene, index


class Scene:
    """Scene(diffLightColor, diffLightPower) -- Scene.cpp:10-71."""

    def __init__(self, diffLightColor: Color = Color(0, 0, 0), diffLightPower: float = 0.0):
        L = _lib.load()
        self._h = C.c_void_p(L.rfx_scene_create(*Color(*diffLightColor), float(diffLightPower)))
        if not self._h:
            raise _lib.RfxError("rfx_scene_create failed")
        self._version = 0
        self._keep = []

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib._lib is not None:
            _lib._lib.rfx_scene_destroy(h)
            self._h = None

    def addSphere(self, center: Vector3, radius: float, material: Material) -> Sphere:
        obj = check(_lib.load().rfx_scene_add_sphere(self._h, farr(Vector3(*center)), float(radius), material.type,
                                                     farr(material.color), material.reflectivity, material.transparency),
                    "Scene.addSphere")
        self._version += 1
        return Sphere(self, obj)

    def addTriangle(self, v1: Vector3, v2: Vector3, v3: Vector3, material: Material) -> Triangle:
        obj = check(_lib.load().rfx_scene_add_triangle(self._h, farr(Vector3(*v1)), farr(Vector3(*v2)), farr(Vector3(*v3)),
                                                       material.type, farr(material.color), material.reflectivity,
                                                       material.transparency), "Scene.addTriangle")
        self._version += 1
        return Triangle(self, obj)

    def addMesh(self, vertices, indices, material: Material) -> List[Triangle]:
        """A triangle mesh in one call (rfx.h rfx_scene_add_mesh): vertices (n, 3) floats, indices (m, 3) vertex
        numbers; the same as m addTriangle calls in index order.  Returns the m Triangle handles."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        first = check(_lib.load().rfx_scene_add_mesh(self._h, _lib.fptr(v), v.shape[0], _lib.u32ptr(i), i.shape[0],
                                                     material.type, farr(material.color), material.reflectivity,
                                                     material.transparency), "Scene.addMesh")
        self._version += 1
        return [Triangle(self, first + k) for k in range(i.shape[0])]

    def tri_bvh_dump(self):
        """The triangle BVH a renderer would build for this scene (rfx.h rfx_scene_tri_bvh_dump; host only), or None
        without one: dict of nodes, leaves, leaf_size, depth, boxes (nodes, 2, 6), children (nodes, 2), leaf_ids
        (leaves, leaf_size), residual."""
        L = _lib.load()
        cnt = (C.c_int32 * 5)()
        if check(L.rfx_scene_tri_bvh_dump(self._h, cnt, None, None, None, None), "Scene.tri_bvh_dump") == 0:
            return None
        nodes, leaves, nres, leaf, depth = (int(x) for x in cnt)
        boxes = np.zeros((nodes, 2, 6), np.float32)
        children = np.zeros((nodes, 2), np.int32)
        ids = np.zeros((leaves, leaf), np.int32)
        res = np.zeros(nres, np.int32)
        i32 = lambda a: a.ctypes.data_as(_lib._i32p)
        check(L.rfx_scene_tri_bvh_dump(self._h, cnt, _lib.fptr(boxes), i32(children), i32(ids), i32(res)),
              "Scene.tri_bvh_dump")
        return {"nodes": nodes, "leaves": leaves, "leaf_size": leaf, "depth": depth, "boxes": boxes,
                "children": children, "leaf_ids": ids, "residual": res}

    def setTriangleVertices(self, first: int, vertices):
        """New vertices for triangles [first, first + n) (rfx.h rfx_scene_set_triangle_vertices): (n, 3, 3) floats, each
        triangle's (v1, v2, v3) as addTriangle takes them.  Materials, textures and uv stay; the next upload of the scene
        reads them."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 9)
        check(_lib.load().rfx_scene_set_triangle_vertices(self._h, int(first), v.shape[0], _lib.fptr(v)),
              "Scene.setTriangleVertices")
        self._version += 1

    def object_triangle(self, obj: int) -> int:
        """The triangle index (insertion order among triangles) of object `obj` (rfx.h rfx_scene_object_triangle)."""
        return check(_lib.load().rfx_scene_object_triangle(self._h, int(obj)), "Scene.object_triangle")

    def tri_records(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The words that follow the triangles' vertices (rfx.h rfx_scene_tri_records; host only): (count,
        RFX_TRI_RECORD_WORDS) uint32."""
        n = self.counts()[1] - first if count is None else count
        out = np.zeros((n, _lib.RFX_TRI_RECORD_WORDS), np.uint32)
        check(_lib.load().rfx_scene_tri_records(self._h, int(first), n, _lib.u32ptr(out)), "Scene.tri_records")
        return out

    def tri_bvh_refit(self, vertices, widen: bool):
        """This scene's triangle BVH refitted on the host to `vertices` ((triangles, 3, 3) floats), as the device update
        refits it (rfx.h rfx_scene_tri_bvh_refit): (boxes (nodes, 2, 6), mt (nodes, 2)), or None without a tree."""
        d = self.tri_bvh_dump()
        if d is None:
            return None
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 9)
        if v.shape[0] != self.counts()[1]:
            raise ValueError("tri_bvh_refit: vertices for every triangle of the scene")
        boxes, mt = np.zeros((d["nodes"], 2, 6), np.float32), np.zeros((d["nodes"], 2), np.float32)
        check(_lib.load().rfx_scene_tri_bvh_refit(self._h, _lib.fptr(v), int(bool(widen)), _lib.fptr(boxes),
                                                  _lib.fptr(mt)), "Scene.tri_bvh_refit")
        return boxes, mt

    def tri_bvh_recut(self, cut_vertices, vertices=None, widen: bool = False):
        """This scene's triangle BVH re-cut on the host at `cut_vertices` and fitted to `vertices` (None: the cut's), as
        Renderer.recut_triangles does it on the device (rfx.h "Re-cutting", rfx_scene_tri_bvh_recut): tri_bvh_dump's
        dict -- the in-tree set and the residual list stay this scene's -- plus mt (nodes, 2), or None without a tree."""
        d = self.tri_bvh_dump()
        if d is None:
            return None
        n = self.counts()[1]
        cut = np.ascontiguousarray(cut_vertices, dtype=np.float32).reshape(-1, 9)
        fit = cut if vertices is None else np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 9)
        if cut.shape[0] != n or fit.shape[0] != n:
            raise ValueError("tri_bvh_recut: vertices for every triangle of the scene")
        cnt = (C.c_int32 * 5)()
        boxes, mt = np.zeros((d["nodes"], 2, 6), np.float32), np.zeros((d["nodes"], 2), np.float32)
        children, ids = np.zeros((d["nodes"], 2), np.int32), np.zeros((d["leaves"], d["leaf_size"]), np.int32)
        i32 = lambda a: a.ctypes.data_as(_lib._i32p)
        if check(_lib.load().rfx_scene_tri_bvh_recut(self._h, _lib.fptr(cut), None if vertices is None else _lib.fptr(fit),
                                                     int(bool(widen)), cnt, _lib.fptr(boxes), i32(children), i32(ids),
                                                     _lib.fptr(mt)), "Scene.tri_bvh_recut") == 0:
            return None
        assert (cnt[0], cnt[1]) == (d["nodes"], d["leaves"])
        return {"nodes": int(cnt[0]), "leaves": int(cnt[1]), "leaf_size": int(cnt[3]), "depth": int(cnt[4]), "boxes": boxes,
                "children": children, "leaf_ids": ids, "residual": d["residual"], "mt": mt}

    def setSpheres(self, first: int, spheres):
        """New centres and radii for spheres [first, first + n) (rfx.h rfx_scene_set_spheres): (n, 4) floats, centre
        then radius (clamped as addSphere clamps it).  Materials stay; the next upload of the scene reads them."""
        v = np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4)
        check(_lib.load().rfx_scene_set_spheres(self._h, int(first), v.shape[0], _lib.fptr(v)), "Scene.setSpheres")
        self._version += 1

    def object_sphere(self, obj: int) -> int:
        """The sphere index (insertion order among spheres) of object `obj` (rfx.h rfx_scene_object_sphere)."""
        return check(_lib.load().rfx_scene_object_sphere(self._h, int(obj)), "Scene.object_sphere")

    def sph_records(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The words that follow the spheres' centres and radii (rfx.h rfx_scene_sph_records; host only): (count,
        RFX_SPH_RECORD_WORDS) uint32."""
        n = self.counts()[0] - first if count is None else count
        out = np.zeros((n, _lib.RFX_SPH_RECORD_WORDS), np.uint32)
        check(_lib.load().rfx_scene_sph_records(self._h, int(first), n, _lib.u32ptr(out)), "Scene.sph_records")
        return out

    def sph_bvh_dump(self):
        """The pair tree a renderer would build for this scene's spheres (rfx.h rfx_scene_sph_bvh_dump; host only):
        dict of nodes, leaves, leaf_size, depth, boxes (nodes, 2, 6), children (nodes, 2), leaf_ids (leaves, leaf_size)
        and device_index (spheres,); without a tree nodes is 0, the arrays are empty and device_index alone is filled."""
        L = _lib.load()
        cnt = (C.c_int32 * 4)()
        dev = np.zeros(self.counts()[0], np.uint32)
        check(L.rfx_scene_sph_bvh_dump(self._h, cnt, None, None, None, _lib.u32ptr(dev)), "Scene.sph_bvh_dump")
        nodes, leaves, leaf, depth = (int(x) for x in cnt)
        boxes = np.zeros((nodes, 2, 6), np.float32)
        children = np.zeros((nodes, 2), np.int32)
        ids = np.zeros((leaves, leaf), np.int32)
        i32 = lambda a: a.ctypes.data_as(_lib._i32p)
        if nodes:
            check(L.rfx_scene_sph_bvh_dump(self._h, cnt, _lib.fptr(boxes), i32(children), i32(ids), None),
                  "Scene.sph_bvh_dump")
        return {"nodes": nodes, "leaves": leaves, "leaf_size": leaf, "depth": depth, "boxes": boxes,
                "children": children, "leaf_ids": ids, "device_index": dev}

    def sph_bvh_refit(self, spheres, widen: bool):
        """This scene's pair tree refitted on the host to `spheres` ((spheres, 4) floats: centre, radius), as the device
        update refits it (rfx.h rfx_scene_sph_bvh_refit): (boxes (nodes, 2, 6), mt (nodes, 2), chunk_bounds (chunks, 4));
        without a tree the first two are empty."""
        L = _lib.load()
        n = self.counts()[0]
        v = np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4)
        if v.shape[0] != n:
            raise ValueError("sph_bvh_refit: a centre and radius for every sphere of the scene")
        cnt = (C.c_int32 * 4)()
        check(L.rfx_scene_sph_bvh_dump(self._h, cnt, None, None, None, None), "Scene.sph_bvh_dump")
        boxes, mt = np.zeros((cnt[0], 2, 6), np.float32), np.zeros((cnt[0], 2), np.float32)
        chunks = np.zeros(((n + 63) // 64, 4), np.float32)
        check(L.rfx_scene_sph_bvh_refit(self._h, _lib.fptr(v), int(bool(widen)), _lib.fptr(boxes), _lib.fptr(mt),
                                        _lib.fptr(chunks)), "Scene.sph_bvh_refit")
        return boxes, mt, chunks

    def cull_dump(self):
        """The bundle-cull records of a small scene as a renderer would upload them (rfx.h rfx_scene_cull_dump; host
        only): (recs (64, 8), tris (32, 12), valid lanes as an int)."""
        recs, tris = np.zeros((64, 8), np.float32), np.zeros((32, 12), np.float32)
        valid = C.c_uint64(0)
        check(_lib.load().rfx_scene_cull_dump(self._h, _lib.fptr(recs), _lib.fptr(tris), C.byref(valid)), "Scene.cull_dump")
        return recs, tris, int(valid.value)

    def set_tri_mates(self, on: bool):
        """Group coplanar triangles whose plane crossing is one value per ray (rfx.h rfx_scene_set_tri_mates): on by
        default; off makes every triangle its own group.  No pixel changes; read by the next upload of the scene."""
        check(_lib.load().rfx_scene_set_tri_mates(self._h, int(bool(on))), "Scene.set_tri_mates")
        self._version += 1

    def tri_mates(self, plane: bool = False):
        """Each triangle's mate-group leader, the lowest triangle index of its group (rfx.h rfx_scene_tri_mates; host
        only); plane: also the (triangles, 6) float32 rows v0 x y z, a31 a32 a33 that the grouping rule compares."""
        L = _lib.load()
        n = check(L.rfx_scene_tri_mates(self._h, None, None), "Scene.tri_mates")
        leader, rows = np.zeros(n, np.int32), np.zeros((n, 6), np.float32)
        check(L.rfx_scene_tri_mates(self._h, leader.ctypes.data_as(_lib._i32p), _lib.fptr(rows)), "Scene.tri_mates")
        return (leader, rows) if plane else leader

    def set_far_lights(self, mode: int):
        """Far-light kernels (rfx.h rfx_scene_set_far_lights): 0 never, 1 automatic (the default), 2 for any one-light
        scene whose light is far.  No pixel changes; read by the next upload of the scene."""
        check(_lib.load().rfx_scene_set_far_lights(self._h, int(mode)), "Scene.set_far_lights")
        self._version += 1

    def far_light(self, light: int = 0):
        """(chosen, terms): whether this scene's launches take the far-light kernels, and light `light`'s record terms
        as float32 [dlen, ndx, ndy, ndz, spec_add, near, cone_cos, cone_sin] (rfx.h rfx_scene_far_light; host only)."""
        terms = np.zeros(8, np.float32)
        chosen = check(_lib.load().rfx_scene_far_light(self._h, int(light), _lib.fptr(terms)), "Scene.far_light")
        return bool(chosen), terms

    def set_shadow_grid(self, mode: int):
        """A far light's occluder grid (rfx.h rfx_scene_set_shadow_grid): 0 none, 1 where the far-light kernels run (the
        default), 2 for any small scene with one far light.  No pixel changes; read by the next upload of the scene."""
        check(_lib.load().rfx_scene_set_shadow_grid(self._h, int(mode)), "Scene.set_shadow_grid")
        self._version += 1

    def shadow_grid(self):
        """The occluder grid a renderer would upload for this scene (rfx.h rfx_scene_shadow_grid; host only), or None
        without one: dict of origin (3,) float32, scale, cell, ball (float32), dims (nx, ny, nz), masks (nz, ny, nx)
        uint64."""
        L = _lib.load()
        n = check(L.rfx_scene_shadow_grid(self._h, None, None, None, 0), "Scene.shadow_grid")
        if n == 0:
            return None
        geom, dims, masks = np.zeros(6, np.float32), np.zeros(3, np.int32), np.zeros(n, np.uint64)
        check(L.rfx_scene_shadow_grid(self._h, _lib.fptr(geom), dims.ctypes.data_as(_lib._i32p), _lib.u64ptr(masks), n),
              "Scene.shadow_grid")
        nx, ny, nz = (int(v) for v in dims)
        return {"origin": geom[:3].copy(), "scale": geom[3], "cell": geom[4], "ball": geom[5], "dims": (nx, ny, nz),
                "masks": masks.reshape(nz, ny, nx)}

    def addPlane(self, pos: Vector3, norm: Vector3, material: Material) -> Plane:
        """Plane(pos, norm, material) (Plane.cpp:9-14) as a scene object, traced by Plane::trace (Plane.cpp:36-73)."""
        obj = check(_lib.load().rfx_scene_add_plane(self._h, farr(Vector3(*pos)), farr(Vector3(*norm)), material.type,
                                                    farr(material.color), material.reflectivity, material.transparency),
                    "Scene.addPlane")
        self._version += 1
        return Plane(self, obj)

    def addLight(self, origin: Vector3, radius: float, color: Color, power: float) -> OmniLight:
        idx = check(_lib.load().rfx_scene_add_light(self._h, farr(Vector3(*origin)), float(radius), farr(Color(*color)),
                                                    float(power)), "Scene.addLight")
        self._version += 1
        return OmniLight(self, idx)

    def addTexture(self, fileName: str) -> Texture:
        """Scene::addTexture(fileName): TGA; a failed load gives the checker texture, like the reference."""
        loaded = C.c_int(0)
        idx = check(_lib.load().rfx_scene_add_texture_file(self._h, os.fsencode(fileName), C.byref(loaded)),
                    "Scene.addTexture")
        self._version += 1
        return Texture(self, idx, bool(loaded.value))

    def addTextureArgb(self, argb: Optional[np.ndarray]) -> Texture:
        """Texture from an (h, w) uint32 ARGB array; None = empty (checker)."""
        L = _lib.load()
        if argb is None:
            idx = check(L.rfx_scene_add_texture_argb(self._h, 0, 0, None), "Scene.addTextureArgb")
        else:
            a = np.ascontiguousarray(argb, dtype=np.uint32)
            idx = check(L.rfx_scene_add_texture_argb(self._h, a.shape[1], a.shape[0], _lib.u32ptr(a)), "Scene.addTextureArgb")
        self._version += 1
        return Texture(self, idx, argb is not None)

    def setSkyboxTexture(self, fileName: str) -> bool:
        ok = check(_lib.load().rfx_scene_set_skybox_file(self._h, os.fsencode(fileName)), "Scene.setSkyboxTexture")
        self._version += 1
        return bool(ok)

    def setSkyboxTextureArgb(self, argb: Optional[np.ndarray]) -> bool:
        L = _lib.load()
        if argb is None:
            ok = check(L.rfx_scene_set_skybox_argb(self._h, 0, 0, None), "Scene.setSkyboxTextureArgb")
        else:
            a = np.ascontiguousarray(argb, dtype=np.uint32)
            ok = check(L.rfx_scene_set_skybox_argb(self._h, a.shape[1], a.shape[0], _lib.u32ptr(a)), "Scene.setSkyboxTextureArgb")
        self._version += 1
        return bool(ok)

    def counts(self):
        v = [C.c_int() for _ in range(4)]
        check(_lib.load().rfx_scene_counts(self._h, *[C.byref(x) for x in v]), "Scene.counts")
        return tuple(x.value for x in v)


def build_scene(desc, texture_dir: Optional[str] = None) -> tuple:
    """Replay a :class:`reflaxman_amd.scenes.SceneDesc` through the Scene API; returns (Scene, Camera).

    texture_dir: write the textures as TGA files there (SceneDesc.write) and load them through
    Scene.addTexture / setSkyboxTexture (the library's TGA reader), as the reference's loadScene does."""
    d = desc.diffuse
    s = Scene(Color(d[0], d[1], d[2]), d[3])
    files = {}
    if texture_dir is not None:
        path = desc.write(texture_dir)
        for line in open(path):
            parts = line.split()
            if parts and parts[0] in ("skybox", "texture"):
                files.setdefault(parts[0], []).append(
                    None if parts[1] == "-" else os.path.join(texture_dir, parts[1]))
    if desc.skybox is not None:
        if texture_dir is not None:
            s.setSkyboxTexture(files["skybox"][0] or "/nonexistent/absent.tga")
        else:
            s.setSkyboxTextureArgb(desc.skybox.argb)
    for (o, r, c, p) in desc.lights:
        s.addLight(Vector3(*o), r, Color(*c), p)
    if texture_dir is not None:
        texs = [s.addTexture(f or "/nonexistent/absent.tga") for f in files.get("texture", [])]
    else:
        texs = [s.addTextureArgb(t.argb) for t in desc.textures]
    handles = []
    for ob in desc.objects:
        mt, rgb, refl, tr = ob[-1]
        m = Material(mt, Color(*rgb), refl, tr)
        if ob[0] == "sphere":
            handles.append(s.addSphere(Vector3(*ob[1]), ob[2], m))
        elif ob[0] == "plane":
            handles.append(s.addPlane(Vector3(*ob[1]), Vector3(*ob[2]), m))
        else:
            handles.append(s.addTriangle(Vector3(*ob[1]), Vector3(*ob[2]), Vector3(*ob[3]), m))
    for (oi, ti, uv) in desc.settex:
        handles[oi].setTexture(texs[ti], *uv)
    eye, at, fov = desc.camera
    return s, Camera(Vector3(*eye), Vector3(*at), fov)


class Renderer:
    """Thin owner of an rfx_renderer (device, stream, uploaded scene, RNG streams)."""

    def __init__(self, device: int = 0, sphere_seed: int = DEFAULT_SPHERE_SEED, jitter_seed: int = DEFAULT_JITTER_SEED):
        L = _lib.load()
        h = C.c_void_p()
        check(L.rfx_renderer_create(C.byref(h), int(device)), "rfx_renderer_create")
        self._h = h
        self.device = device
        self._scene_key = None
        self.set_rng(sphere_seed, jitter_seed)

    def close(self):
        if getattr(self, "_h", None) and _lib._lib is not None:
            _lib._lib.rfx_renderer_destroy(self._h)
            self._h = None

    __del__ = close

    def set_scene(self, scene: Scene):
        key = (id(scene), scene._version)
        if key != self._scene_key:
            check(_lib.load().rfx_renderer_set_scene(self._h, scene._h), "rfx_renderer_set_scene")
            self._scene_key = key
            self._scene_ref = scene

    def update_triangles(self, first: int, positions, indices=None):
        """New vertices for triangles [first, first + n) of the uploaded scene, on the device (rfx.h "Moving meshes",
        rfx_renderer_update_triangles): every later launch is the one a renderer gives whose set_scene got the scene
        built at these vertices.  positions: (n, 3, 3) floats, each triangle's three vertices -- or, with indices (n, 3),
        a vertex pool (m, 3) the index triples name (a triangle naming an index >= m keeps its vertices).  Torch tensors
        on this renderer's device are read where they lie, on torch's current stream, with no host sync (trace_rays'
        conventions); anything else goes through numpy and the host form, which synchronises.  A small scene raises
        (set_scene uploads it again).  A later set_scene(scene) uploads again: move the Scene too
        (Scene.setTriangleVertices) if it is to match."""
        L = _lib.load()
        try:
            import torch
            is_torch = isinstance(positions, torch.Tensor)
        except ImportError:
            is_torch = False
        self._scene_key = None
        if is_torch:
            if not positions.is_cuda or positions.device.index != self.device:
                raise ValueError("update_triangles: tensors on the renderer's device (or numpy arrays) are required")
            p = positions.to(torch.float32).reshape(-1, 3).contiguous()
            idx = None
            if indices is not None:
                if not (isinstance(indices, torch.Tensor) and indices.is_cuda and indices.device == positions.device):
                    raise ValueError("update_triangles: indices on the positions' device")
                # (uint32 words: torch has no unsigned kind on every build; a negative int32 names no vertex either way)
                idx = indices.to(torch.int32).reshape(-1, 3).contiguous()
            n = idx.shape[0] if idx is not None else p.shape[0] // 3
            stream = torch.cuda.current_stream(p.device).cuda_stream
            if not stream:
                torch.cuda.current_stream(p.device).synchronize()
            check(L.rfx_renderer_update_triangles(self._h, int(first), n, C.c_void_p(p.data_ptr()), p.shape[0],
                                                  C.c_void_p(idx.data_ptr() if idx is not None else None),
                                                  C.c_void_p(stream or None)), "rfx_renderer_update_triangles")
            if not stream:
                self.synchronize()
            else:
                self._keep_update = (p, idx)  # the launch reads them after this call returns
            return
        p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        n = idx.shape[0] if idx is not None else p.shape[0] // 3
        check(L.rfx_renderer_update_triangles_host(self._h, int(first), n, _lib.fptr(p), p.shape[0],
                                                   _lib.u32ptr(idx) if idx is not None else None),
              "rfx_renderer_update_triangles_host")

    def recut_triangles(self, stream=None):
        """Re-cut the uploaded triangle BVH at the triangles' current vertices, on the device (rfx.h "Re-cutting",
        rfx_renderer_recut_triangles): no value of any launch changes, only how fast a moved mesh is traced.
        Stream-ordered with no host sync: stream is a raw stream pointer as render_frame takes it (an update from torch
        tensors runs on torch's current stream: pass that one), None the renderer's own.  Raises without a triangle
        tree."""
        self._scene_key = None  # (as after an update: a later set_scene(scene) uploads again, and restores the built tree)
        check(_lib.load().rfx_renderer_recut_triangles(self._h, C.c_void_p(stream or None)),
              "rfx_renderer_recut_triangles")

    def tri_records(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The uploaded triangles' words that follow their vertices, read back (rfx.h rfx_renderer_tri_records;
        synchronises): (count, RFX_TRI_RECORD_WORDS) uint32."""
        n = self._scene_ref.counts()[1] - first if count is None else count
        out = np.zeros((n, _lib.RFX_TRI_RECORD_WORDS), np.uint32)
        check(_lib.load().rfx_renderer_tri_records(self._h, int(first), n, _lib.u32ptr(out)), "rfx_renderer_tri_records")
        return out

    def tri_bvh_nodes(self):
        """The uploaded triangle BVH read back (rfx.h rfx_renderer_tri_bvh_nodes; synchronises): (boxes (nodes, 2, 6)
        float32, children (nodes, 2) int32, mt (nodes, 2) float32), or None without a tree."""
        L = _lib.load()
        n = check(L.rfx_renderer_tri_bvh_nodes(self._h, None), "rfx_renderer_tri_bvh_nodes")
        if n == 0:
            return None
        out = np.zeros((n, 16), np.float32)
        check(L.rfx_renderer_tri_bvh_nodes(self._h, _lib.fptr(out)), "rfx_renderer_tri_bvh_nodes")
        return out[:, :12].reshape(n, 2, 6).copy(), out[:, 12:14].copy().view(np.int32), out[:, 14:16].copy()

    def tri_leaves(self):
        """The uploaded triangle BVH's leaves read back (rfx.h rfx_renderer_tri_leaves; synchronises): (leaf_ids
        (leaves, 4) int32, slot (triangles,) int32, records (slots, 14) uint32 by position), or None without a tree."""
        L = _lib.load()
        slots = check(L.rfx_renderer_tri_leaves(self._h, None, None, None), "rfx_renderer_tri_leaves")
        if slots == 0:
            return None
        leaf = self.accel_info().tri_leaf_size
        ids = np.zeros((slots // leaf, leaf), np.int32)
        slot = np.zeros(self._scene_ref.counts()[1], np.int32)
        rec = np.zeros((slots, 14), np.uint32)
        i32 = lambda a: a.ctypes.data_as(_lib._i32p)
        check(L.rfx_renderer_tri_leaves(self._h, i32(ids), i32(slot), _lib.u32ptr(rec)), "rfx_renderer_tri_leaves")
        return ids, slot, rec

    def update_spheres(self, first: int, spheres, ids=None):
        """New centres and radii for spheres of the uploaded scene, on the device (rfx.h "Moving spheres",
        rfx_renderer_update_spheres): every later launch is the one a renderer gives whose set_scene got the scene built
        at these spheres.  spheres: (n, 4) floats, centre then radius, for spheres [first, first + n) of the insertion
        order -- or, with ids (n,), for the spheres the ids name (`first` is ignored; an id beyond the scene's spheres is
        skipped).  Torch tensors on this renderer's device are read where they lie, on torch's current stream, with no
        host sync (update_triangles' conventions); anything else goes through numpy and the host form, which
        synchronises.  A small scene raises.  A later set_scene(scene) uploads again: move the Scene too
        (Scene.setSpheres) if it is to match."""
        L = _lib.load()
        try:
            import torch
            is_torch = isinstance(spheres, torch.Tensor)
        except ImportError:
            is_torch = False
        self._scene_key = None
        if is_torch:
            if not spheres.is_cuda or spheres.device.index != self.device:
                raise ValueError("update_spheres: tensors on the renderer's device (or numpy arrays) are required")
            p = spheres.to(torch.float32).reshape(-1, 4).contiguous()
            idx = None
            if ids is not None:
                if not (isinstance(ids, torch.Tensor) and ids.is_cuda and ids.device == spheres.device):
                    raise ValueError("update_spheres: ids on the spheres' device")
                idx = ids.to(torch.int32).reshape(-1).contiguous()  # (uint32 words: a negative int32 names no sphere)
                if idx.shape[0] != p.shape[0]:
                    raise ValueError("update_spheres: one id per sphere record")
            stream = torch.cuda.current_stream(p.device).cuda_stream
            if not stream:
                torch.cuda.current_stream(p.device).synchronize()
            check(L.rfx_renderer_update_spheres(self._h, int(first), p.shape[0], C.c_void_p(p.data_ptr()),
                                                C.c_void_p(idx.data_ptr() if idx is not None else None),
                                                C.c_void_p(stream or None)), "rfx_renderer_update_spheres")
            if not stream:
                self.synchronize()
            else:
                self._keep_update = (p, idx)  # the launch reads them after this call returns
            return
        p = np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4)
        idx = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if idx is not None and idx.shape[0] != p.shape[0]:
            raise ValueError("update_spheres: one id per sphere record")
        check(L.rfx_renderer_update_spheres_host(self._h, int(first), p.shape[0], _lib.fptr(p),
                                                 _lib.u32ptr(idx) if idx is not None else None),
              "rfx_renderer_update_spheres_host")

    def sph_records(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The uploaded spheres' words that follow their centres and radii, read back in insertion order (rfx.h
        rfx_renderer_sph_records; synchronises): (count, RFX_SPH_RECORD_WORDS) uint32."""
        n = self._scene_ref.counts()[0] - first if count is None else count
        out = np.zeros((n, _lib.RFX_SPH_RECORD_WORDS), np.uint32)
        check(_lib.load().rfx_renderer_sph_records(self._h, int(first), n, _lib.u32ptr(out)), "rfx_renderer_sph_records")
        return out

    def sph_bvh_nodes(self):
        """The uploaded pair tree read back (rfx.h rfx_renderer_sph_bvh_nodes; synchronises): (boxes (nodes, 2, 6)
        float32, children (nodes, 2) int32, mt (nodes, 2) float32), or None without a tree."""
        L = _lib.load()
        n = check(L.rfx_renderer_sph_bvh_nodes(self._h, None), "rfx_renderer_sph_bvh_nodes")
        if n == 0:
            return None
        out = np.zeros((n, 16), np.float32)
        check(L.rfx_renderer_sph_bvh_nodes(self._h, _lib.fptr(out)), "rfx_renderer_sph_bvh_nodes")
        return out[:, :12].reshape(n, 2, 6).copy(), out[:, 12:14].copy().view(np.int32), out[:, 14:16].copy()

    def sph_chunk_bounds(self) -> np.ndarray:
        """The uploaded 64-sphere chunks' bounds read back (rfx.h rfx_renderer_sph_chunk_bounds; synchronises):
        (chunks, 4) float32."""
        L = _lib.load()
        n = check(L.rfx_renderer_sph_chunk_bounds(self._h, None), "rfx_renderer_sph_chunk_bounds")
        out = np.zeros((n, 4), np.float32)
        if n:
            check(L.rfx_renderer_sph_chunk_bounds(self._h, _lib.fptr(out)), "rfx_renderer_sph_chunk_bounds")
        return out

    def sph_padding(self) -> np.ndarray:
        """The padding lanes of the uploaded pair records (rfx.h rfx_renderer_sph_padding; synchronises): (lanes, 4)
        uint32 -- no update writes them."""
        L = _lib.load()
        n = check(L.rfx_renderer_sph_padding(self._h, None), "rfx_renderer_sph_padding")
        out = np.zeros((n, 4), np.uint32)
        if n:
            check(L.rfx_renderer_sph_padding(self._h, _lib.u32ptr(out)), "rfx_renderer_sph_padding")
        return out

    def set_rng(self, sphere_seed: int, jitter_seed: int):
        check(_lib.load().rfx_renderer_set_rng(self._h, sphere_seed & 0xFFFFFFFF, jitter_seed & 0xFFFFFFFF), "set_rng")

    def get_rng(self):
        s, j = C.c_uint32(), C.c_uint32()
        check(_lib.load().rfx_renderer_get_rng(self._h, C.byref(s), C.byref(j)), "get_rng")
        return s.value, j.value

    def set_stream(self, stream_ptr: int):
        check(_lib.load().rfx_renderer_set_stream(self._h, C.c_void_p(stream_ptr)), "set_stream")

    def render_frame(self, frame: _lib.Frame, d_rgb: int, d_argb: int = 0, d_counters: int = 0, stream: int = 0):
        """Enqueue one frame into caller-owned device buffers (device pointers as ints)."""
        check(_lib.load().rfx_render_frame(self._h, C.byref(frame), C.c_void_p(d_rgb), C.c_void_p(d_argb or None),
                                           C.c_void_p(d_counters or None), C.c_void_p(stream or None)), "rfx_render_frame")

    def synchronize(self):
        check(_lib.load().rfx_synchronize(self._h), "rfx_synchronize")

    class _DeviceArrays:
        """Device arrays of a numpy call that has no host form (the ordered calls), from the library's own helpers
        (rfx_device_alloc, rfx_memcpy_h2d / _d2h on the renderer's stream); freed on exit."""

        def __init__(self, renderer):
            self.r, self.L, self.ptrs = renderer, _lib.load(), []

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.L.rfx_synchronize(self.r._h)  # (what was enqueued reads and writes the arrays before they go)
            for p in self.ptrs:
                self.L.rfx_device_free(self.r._h, p)
            return False

        def alloc(self, nbytes: int) -> C.c_void_p:
            p = C.c_void_p()
            check(self.L.rfx_device_alloc(self.r._h, int(nbytes), C.byref(p)), "rfx_device_alloc")
            self.ptrs.append(p)
            return p

        def put(self, a: np.ndarray) -> C.c_void_p:
            p = self.alloc(a.nbytes)
            check(self.L.rfx_memcpy_h2d(self.r._h, p, a.ctypes.data_as(C.c_void_p), a.nbytes), "rfx_memcpy_h2d")
            return p

        def get(self, a: np.ndarray, p) -> np.ndarray:
            check(self.L.rfx_memcpy_d2h(self.r._h, a.ctypes.data_as(C.c_void_p), p, a.nbytes), "rfx_memcpy_d2h")
            return a

    def order_box(self):
        """(lo, scale) of the coherent order's key box for the uploaded scene, float32 (3,) each (rfx.h)."""
        lo, scale = np.empty(3, np.float32), np.empty(3, np.float32)
        check(_lib.load().rfx_renderer_order_box(self._h, _lib.fptr(lo), _lib.fptr(scale)), "rfx_renderer_order_box")
        return lo, scale

    def order_rays(self, rays, keys: bool = False):
        """The coherent order of a batch (rfx.h rfx_rays_order): the permutation of [0, n) that sorts the rays by their
        key of origin cell and direction, equal keys in index order -- pass it as ``order=`` to trace_rays, query_hits
        or occluded.  ``rays`` as for trace_rays: a torch tensor on this renderer's device is sorted where it lies, on
        torch's current stream, and an int32 tensor comes back; anything else goes through numpy and the host form
        (uint32).  keys: also return every ray's key in ray order, as (order, keys) -- the same bits as int32 in torch."""
        L = _lib.load()
        is_torch, r, stream = self._ray_batch(rays, "order_rays")
        n = r.shape[0]
        if is_torch:
            import torch
            order = torch.empty(n, dtype=torch.int32, device=r.device)
            k = torch.empty(n, dtype=torch.int32, device=r.device) if keys else None
            check(L.rfx_rays_order(self._h, C.c_void_p(r.data_ptr()), n, C.c_void_p(order.data_ptr()),
                                   C.c_void_p(k.data_ptr() if keys else None), C.c_void_p(stream or None)), "rfx_rays_order")
            if not stream:
                self.synchronize()
            return (order, k) if keys else order
        order = np.empty(n, np.uint32)
        k = np.empty(n, np.uint32) if keys else None
        check(L.rfx_rays_order_host(self._h, _lib.fptr(r), n, _lib.u32ptr(order), _lib.u32ptr(k) if keys else None),
              "rfx_rays_order_host")
        return (order, k) if keys else order

    def _order_tensor(self, order, r, what):
        """``order=`` of a torch call as an int32 device tensor of r's n indices ("coherent": order_rays)."""
        import torch
        if isinstance(order, str):
            if order != "coherent":
                raise ValueError(f"{what}: order is an index array or \"coherent\"")
            return self.order_rays(r)
        if isinstance(order, torch.Tensor):
            o = order.to(device=r.device, dtype=torch.int32).reshape(-1).contiguous()
        else:
            o = torch.from_numpy(np.ascontiguousarray(order).astype(np.uint32).view(np.int32).reshape(-1)).to(r.device)
        if o.numel() != r.shape[0]:
            raise ValueError(f"{what}: one order entry per ray")
        return o

    def _order_array(self, dev, order, d_rays, n, what) -> C.c_void_p:
        """``order=`` of a numpy call as a device array of n uint32 ("coherent": rfx_rays_order on the device rays)."""
        if isinstance(order, str):
            if order != "coherent":
                raise ValueError(f"{what}: order is an index array or \"coherent\"")
            d_order = dev.alloc(4 * n)
            check(dev.L.rfx_rays_order(self._h, d_rays, n, d_order, None, None), "rfx_rays_order")
            return d_order
        o = np.ascontiguousarray(order).astype(np.uint32).reshape(-1)
        if o.size != n:
            raise ValueError(f"{what}: one order entry per ray")
        return dev.put(o)

    def trace_rays(self, rays, depth: int, raster_width: int = 0, argb: bool = False, counters=None, order=None):
        """Scene::trace on a batch of rays (rfx.h rfx_trace_rays): ``rays`` is (n, 6) float32 -- origin xyz, then the
        direction xyz, used as given -- and the result the (n, 3) float32 colours, ray i's from the i-th
        randomInsideSphere draw of the sphere stream.  A torch tensor on this renderer's device is traced where it
        lies, on torch's current stream, with no host copy (and, off the legacy default stream, no synchronisation), and a
        tensor comes back; anything
        else goes through numpy and the host form (rfx_trace_rays_host), which synchronises.  argb: also return
        Color::argb of every colour, as (colours, words) -- uint32 (numpy) or the same bits as int32 (torch).
        counters: the stats kernel's RFX_NCOUNTERS event counters are added to it -- a numpy uint64 array, or a torch
        int64 tensor on the device.  raster_width W > 0 lays the batch out as a row-major W-wide raster and gives each
        wave an 8x8 tile of it (rays from a camera model); it changes the schedule only, never a value.  order: the
        schedule as an index array instead (rfx.h rfx_trace_rays_ordered) -- wave w traces the rays order[64 w .. 64 w +
        63]; a tensor or array of the n indices, a permutation of [0, n), or "coherent", which takes order_rays(rays)
        first.  Every colour and the stream's end state stay the unordered call's.  Not with raster_width or counters."""
        L = _lib.load()
        if order is not None and (raster_width or counters is not None):
            raise ValueError("trace_rays: order goes with neither raster_width nor counters")
        # on any stream but the legacy default one a device tensor is traced asynchronously; that one has no handle to
        # pass on (NULL is the renderer's own stream, which is not ordered with it): there the call is fenced on both
        # sides instead, its start by _ray_batch and its end below
        is_torch, r, stream = self._ray_batch(rays, "trace_rays")
        n = r.shape[0]
        if is_torch:
            import torch
            rgb = torch.empty((n, 3), dtype=torch.float32, device=r.device)
            words = torch.empty(n, dtype=torch.int32, device=r.device) if argb else None
            if counters is not None and not (isinstance(counters, torch.Tensor) and counters.is_cuda and
                                             counters.dtype == torch.int64 and counters.is_contiguous() and
                                             counters.numel() >= _lib.RFX_NCOUNTERS):
                raise ValueError("trace_rays: counters must be a contiguous int64 device tensor of RFX_NCOUNTERS words")
            if order is not None:
                o = self._order_tensor(order, r, "trace_rays")
                check(L.rfx_trace_rays_ordered(self._h, C.c_void_p(r.data_ptr()), C.c_void_p(o.data_ptr()), n, int(depth),
                                               C.c_void_p(rgb.data_ptr()), C.c_void_p(words.data_ptr() if argb else None),
                                               C.c_void_p(stream or None)), "rfx_trace_rays_ordered")
            else:
                check(L.rfx_trace_rays(self._h, C.c_void_p(r.data_ptr()), n, int(depth), int(raster_width),
                                       C.c_void_p(rgb.data_ptr()), C.c_void_p(words.data_ptr() if argb else None),
                                       C.c_void_p(counters.data_ptr() if counters is not None else None),
                                       C.c_void_p(stream or None)), "rfx_trace_rays")
            if not stream:
                self.synchronize()
            return (rgb, words) if argb else rgb
        rgb = np.empty((n, 3), np.float32)
        words = np.empty(n, np.uint32) if argb else None
        if counters is not None and not (isinstance(counters, np.ndarray) and counters.dtype == np.uint64 and
                                         counters.flags.c_contiguous and counters.size >= _lib.RFX_NCOUNTERS):
            raise ValueError("trace_rays: counters must be a contiguous uint64 array of RFX_NCOUNTERS words")
        if order is not None:
            with self._DeviceArrays(self) as dev:
                d_rays = dev.put(r)
                d_order = self._order_array(dev, order, d_rays, n, "trace_rays")
                d_rgb, d_argb = dev.alloc(rgb.nbytes), dev.alloc(4 * n) if argb else None
                check(L.rfx_trace_rays_ordered(self._h, d_rays, d_order, n, int(depth), d_rgb, d_argb, None),
                      "rfx_trace_rays_ordered")
                dev.get(rgb, d_rgb)
                if argb:
                    dev.get(words, d_argb)
                self.synchronize()  # (the pre-pass's error word)
            return (rgb, words) if argb else rgb
        check(L.rfx_trace_rays_host(self._h, _lib.fptr(r), n, int(depth), int(raster_width), _lib.fptr(rgb),
                                    _lib.u32ptr(words) if argb else None,
                                    _lib.u64ptr(counters) if counters is not None else None), "rfx_trace_rays_host")
        return (rgb, words) if argb else rgb

    HIT_PLANES = ("object", "distance", "point", "normal", "reflected", "colour")

    def _ray_batch(self, rays, what):
        """(is_torch, the (n, 6) float32 records, torch's current stream handle or None)."""
        try:
            import torch
            is_torch = isinstance(rays, torch.Tensor)
        except ImportError:
            is_torch = False
        if not is_torch:
            return False, np.ascontiguousarray(rays, np.float32).reshape(-1, 6), None
        if not rays.is_cuda or rays.device.index != self.device:
            raise ValueError(f"{what}: a tensor on the renderer's device (or a numpy array) is required")
        r = rays.to(torch.float32).reshape(-1, 6).contiguous()
        # the legacy default stream has no handle to pass on (trace_rays): there the call is fenced on both sides, here
        # and by the caller once it is enqueued
        stream = torch.cuda.current_stream(r.device).cuda_stream
        if not stream:
            torch.cuda.current_stream(r.device).synchronize()
        return True, r, stream

    def _span(self, what, n, is_torch, device, lo=None, after=None, hi=None):
        """The interval arrays of a span query (rfx.h rfx_ray_span) as {end: n-entry array of the kind the rays are},
        or None when no end is given.  A scalar end holds for every ray; ``after`` counts only beside ``lo``."""
        if after is not None and lo is None:
            raise ValueError(f"{what}: after goes with lo")
        if lo is None and hi is None:
            return None
        ends = {}
        for k, v, dt in (("d_lo", lo, "float32"), ("d_after", after, "int32"), ("d_hi", hi, "float32")):
            if v is None:
                continue
            if is_torch:
                import torch
                if isinstance(v, np.ndarray):
                    v = np.array(v)  # (a copy: torch takes no read-only array)
                a = torch.as_tensor(v, device=device).to(getattr(torch, dt)).reshape(-1)
                a = (a.expand(n) if a.numel() == 1 else a).contiguous()
                size = a.numel()
            else:
                a = np.asarray(v, dt).reshape(-1)
                a = np.ascontiguousarray(np.broadcast_to(a, (n,)) if a.size == 1 else a)
                size = a.size
            if size != n:
                raise ValueError(f"{what}: one {k[2:]} entry per ray")
            ends[k] = a
        return ends

    def _query(self, kind, what, is_torch, r, stream, raster_width, order, ends, skip, out):
        """One call of a hit query (query_hits: kind "hits"; occluded: kind "occluded").  The C entry is
        rfx_query_<kind>[_span][_ordered | _host]: _span with an interval (ends, from _span), _ordered with ``order``,
        else _host for numpy arrays.  Tensors are passed where they lie, on ``stream`` (_ray_batch; the legacy stream is
        fenced here); numpy arrays with ``order``, which has no host form, go through _DeviceArrays.  skip: the any-hit's
        array or None; out: the result arrays by name, filled in place -- the planes of "hits" (an rfx_hit_planes), the
        one array of "occluded"."""
        n, host = r.shape[0], not is_torch and order is None
        name = f"rfx_query_{kind}" + ("_span" if ends is not None else "") + (
            "_ordered" if order is not None else "_host" if host else "")
        address = lambda p: C.cast(p, C.c_void_p).value
        with (contextlib.nullcontext() if is_torch or host else self._DeviceArrays(self)) as dev:
            if is_torch:
                src = dst = lambda a: C.c_void_p(a.data_ptr())
            elif host:
                src = dst = lambda a: a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))
            else:
                src, dst = dev.put, lambda a: dev.alloc(a.nbytes)
            d_rays = src(r)
            args = [self._h, d_rays]
            if kind == "occluded":
                args.append(src(skip) if skip is not None else None)
            if ends is not None:
                args.append(C.byref(_lib.RaySpan(**{k: address(src(a)) for k, a in ends.items()})))
            if order is not None:
                o = self._order_tensor(order, r, what) if is_torch else None
                args.append(src(o) if is_torch else self._order_array(dev, order, d_rays, n, what))
            args.append(n)
            if order is None:
                args.append(int(raster_width))
            d_out = {k: dst(a) for k, a in out.items()}
            if kind == "hits":
                args.append(C.byref(_lib.HitPlanes(**{k: address(p) for k, p in d_out.items()})))
            else:
                args.extend(d_out.values())
            if not host:
                args.append(C.c_void_p(stream or None))
            check(getattr(_lib.load(), name)(*args), name)
            if dev is not None:
                for k, a in out.items():
                    dev.get(a, d_out[k])
        if is_torch and not stream:
            self.synchronize()

    def query_hits(self, rays, raster_width: int = 0, want=HIT_PLANES, order=None, lo=None, after=None, hi=None):
        """The closest hit of every ray (rfx.h rfx_query_hits: one pass of Scene.cpp:82-107): a dict of the planes
        named in ``want`` -- object (n, int32, -1 = no hit), distance (n, FLT_MAX on a miss), point, normal, reflected,
        colour ((n, 3), zero on a miss).  ``rays`` as for trace_rays: a torch tensor on this renderer's device is
        queried where it lies, on torch's current stream, and tensors come back; anything else goes through numpy and
        the host form, which synchronises.  No random stream moves.  order: as for trace_rays (rfx.h
        rfx_query_hits_ordered): an index array or "coherent"; not with raster_width.
        lo, after, hi: a per-ray interval (rfx.h "Ray intervals", rfx_query_hits_span) -- the winner is the closest
        candidate with distance <= hi and (distance, object) after (lo, after): after = -1 (the default) includes a
        candidate at lo itself, INT32_MAX excludes it, the previous winner steps to the next object at that distance.
        Arrays of n entries of the kind ``rays`` is, or one number for every ray."""
        if order is not None and raster_width:
            raise ValueError("query_hits: order goes with no raster_width")
        want = tuple(want)
        if not want or any(k not in self.HIT_PLANES for k in want):
            raise ValueError(f"query_hits: want names at least one of {self.HIT_PLANES}")
        is_torch, r, stream = self._ray_batch(rays, "query_hits")
        n = r.shape[0]
        shape = lambda k: (n,) if k in ("object", "distance") else (n, 3)
        if is_torch:
            import torch
            out = {k: torch.empty(shape(k), dtype=torch.int32 if k == "object" else torch.float32, device=r.device)
                   for k in want}
        else:
            out = {k: np.empty(shape(k), np.int32 if k == "object" else np.float32) for k in want}
        ends = self._span("query_hits", n, is_torch, r.device if is_torch else None, lo, after, hi)
        self._query("hits", "query_hits", is_torch, r, stream, raster_width, order, ends, None, out)
        return out

    def occluded(self, rays, skip=None, raster_width: int = 0, order=None, lo=None, hi=None):
        """Whether anything stands in each ray's way (rfx.h rfx_query_occluded, the shadow rays' any-hit of
        Scene.cpp:133-143): (n,) uint8, 1 = some object other than ``skip[i]`` is hit.  Without ``lo`` / ``hi`` (below)
        the ray is unbounded.  skip: (n,) int32 object indices (None, or a value outside [0, objects): nothing is left out), of the kind ``rays``
        is -- a device tensor with a device tensor, else numpy.  order: as for trace_rays (rfx.h
        rfx_query_occluded_ordered): an index array or "coherent"; not with raster_width.
        lo, hi: a per-ray interval (rfx.h rfx_query_occluded_span), both ends inclusive: only objects hit at a distance
        in [lo, hi] count -- the ray becomes a segment.  Arrays of n entries of the kind ``rays`` is, or one number."""
        if order is not None and raster_width:
            raise ValueError("occluded: order goes with no raster_width")
        is_torch, r, stream = self._ray_batch(rays, "occluded")
        n = r.shape[0]
        if is_torch:
            import torch
        sk = None
        if skip is not None:
            if is_torch:
                sk = torch.as_tensor(skip, device=r.device).to(torch.int32).reshape(-1).contiguous()
            else:
                sk = np.ascontiguousarray(skip, np.int32).reshape(-1)
            if (sk.numel() if is_torch else sk.size) != n:
                raise ValueError("occluded: one skip entry per ray")
        occ = torch.empty(n, dtype=torch.uint8, device=r.device) if is_torch else np.empty(n, np.uint8)
        ends = self._span("occluded", n, is_torch, r.device if is_torch else None, lo, None, hi)
        self._query("occluded", "occluded", is_torch, r, stream, raster_width, order, ends, sk, {"occluded": occ})
        return occ

    def query_layers(self, rays, k: int, want=HIT_PLANES, raster_width: int = 0, order=None):
        """The first k layers of every ray (rfx.h "Ray intervals"): a list of k dicts of the planes in ``want``, layer
        0 the closest hit, layer l + 1 the closest candidate after layer l's (distance, object) -- a ray's candidates in
        ascending (distance, index), each once, objects at exactly one distance lower index first.  A ray that has run
        out of candidates is a miss in every later layer.  k calls of query_hits: the stepping planes (object,
        distance) are computed whether wanted or not."""
        if k < 1:
            raise ValueError("query_layers: k >= 1 required")
        want = tuple(want)
        ask = want + tuple(p for p in ("object", "distance") if p not in want)
        layers, lo, after = [], None, None
        for _ in range(int(k)):
            out = self.query_hits(rays, raster_width=raster_width, want=ask, order=order, lo=lo, after=after)
            obj, dist = out["object"], out["distance"]
            # a ray that missed stays out: its lower end becomes +inf, which no candidate lies after
            if isinstance(dist, np.ndarray):
                dist = np.where(obj < 0, np.float32(np.inf), dist)
            else:
                dist = dist.masked_fill(obj < 0, float("inf"))
            layers.append({p: out[p] for p in want})
            lo, after = dist, obj
        return layers

    def visible(self, a, b, skip=None):
        """Whether point b[i] is visible from point a[i]: (n,) uint8, 1 = nothing (but ``skip[i]``) is hit on the
        segment.  The ray is (a, b - a) and its upper end hi = |b - a| as float32 sqrt(dx^2 + dy^2 + dz^2); the far
        end is inclusive -- an object hit at exactly that distance hides b -- and a caller who wants it open passes
        occluded(..., hi=np.nextafter(hi, 0)) itself.  (n, 3) arrays of one kind: device tensors or numpy."""
        try:
            import torch
            is_torch = isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor)
        except ImportError:
            is_torch = False
        if is_torch:
            b = torch.as_tensor(b, dtype=torch.float32, device=a.device if isinstance(a, torch.Tensor) else b.device)
            a = torch.as_tensor(a, dtype=torch.float32, device=b.device).reshape(-1, 3)
            d = b.reshape(-1, 3) - a
            hi = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            return 1 - self.occluded(torch.cat([a, d], dim=1), skip, hi=hi)
        a = np.asarray(a, np.float32).reshape(-1, 3)
        d = np.asarray(b, np.float32).reshape(-1, 3) - a
        hi = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=np.float32)
        return (1 - self.occluded(np.concatenate([a, d], axis=1), skip, hi=hi)).astype(np.uint8)

    def paths(self, rays, draw=True) -> "Paths":
        """The rays as resumable paths (rfx.h "Paths", rfx_paths_begin): a Paths whose step() runs Scene::trace's loop
        segment by segment on state held on the device.  ``rays`` as for trace_rays: a torch tensor on this renderer's
        device starts a torch-backed state with no host copy (the records are copied on the device: a step overwrites
        them), anything else goes through numpy into device arrays of the library's own.  draw: True takes path i's
        randDir from the i-th draw of the sphere stream, as trace_rays does; False leaves the streams alone and gives
        every path the zero vector (the noise-free image); an (n, 3) array gives the caller's own directions."""
        return Paths(self, rays, draw)

    def trace_wavefront(self, rays, depth: int, order=None, argb: bool = False):
        """trace_rays(rays, depth) as a wavefront loop over paths: begin, then a step per segment over the paths still
        live, with order="coherent" the live list sorted by the paths' current rays (Paths.order) before every step but
        the first.  The colours (and words, argb=True) are those of trace_rays, bit for bit, and so is the sphere
        stream's end state; only the schedule differs."""
        if order not in (None, "coherent"):
            raise ValueError("trace_wavefront: order is None or \"coherent\"")
        p = self.paths(rays)
        try:
            live = None
            for k in range(1, int(depth) + 1):
                if live is not None:
                    if len(live) == 0:
                        break
                    if order == "coherent":
                        live = p.order(live)
                live = p.step(k, index=live, live=True)
            return (p.colour, p.argb) if argb else p.colour
        finally:
            p.close()

    def set_tile_order(self, mode: int):
        """Trace-launch schedule (rfx.h rfx_renderer_set_tile_order): 1 longest-tile-first (8x8 wave tiles)
        from earlier launches' tile costs on large launches (default), 3 on every launch, 0 raster order,
        2 raster order with cost recording.  No pixel changes."""
        check(_lib.load().rfx_renderer_set_tile_order(self._h, int(mode)), "set_tile_order")

    def set_prim_masks(self, mode: int):
        """Primary-bundle cull masks of small-scene plain and SSAA frames (rfx.h rfx_renderer_set_prim_masks): 1 built
        when a view repeats (default; sampleNum > 8: every view), 2 before every launch, 0 off.  No pixel changes.  Any
        call forgets the views seen so far."""
        check(_lib.load().rfx_renderer_set_prim_masks(self._h, int(mode)), "set_prim_masks")

    def set_prim_exact(self, on: bool):
        """The per-view masks narrowed to the view's known primary hits (rfx.h rfx_renderer_set_prim_exact): on by
        default; off leaves the conservative bundle culls.  No pixel changes.  Any call drops the masks held."""
        check(_lib.load().rfx_renderer_set_prim_exact(self._h, int(bool(on))), "set_prim_exact")

    def prim_masks(self) -> np.ndarray:
        """The masks held for the current view (rfx.h rfx_renderer_get_prim_masks) as a flat uint64 array -- a small
        scene's: 5 words per 8x8 wave tile, tiles in raster order -- or an empty one when none are held.  Synchronises."""
        L = _lib.load()
        n = C.c_uint64()
        check(L.rfx_renderer_get_prim_masks(self._h, None, 0, C.byref(n)), "get_prim_masks")
        out = np.zeros(n.value, np.uint64)
        if n.value:
            check(L.rfx_renderer_get_prim_masks(self._h, _lib.u64ptr(out), n.value, C.byref(n)), "get_prim_masks")
        return out

    def set_regroup(self, park_after: int):
        """Ray regrouping (rfx.h rfx_renderer_set_regroup): -1 default (large scenes, after 2 segments), 0 off,
        n >= 1 park traces alive after n segments for the packed bounce kernel.  No pixel changes."""
        check(_lib.load().rfx_renderer_set_regroup(self._h, int(park_after)), "set_regroup")

    def set_regroup_sort(self, on: bool):
        """Regrouped frames (rfx.h rfx_renderer_set_regroup_sort): the bounce kernel takes the parked traces sorted
        by direction octant and origin cell, or in park order (default).  No pixel changes."""
        check(_lib.load().rfx_renderer_set_regroup_sort(self._h, int(bool(on))), "set_regroup_sort")

    def set_launch_traces(self, max_traces: int):
        """The most traces one launch takes (rfx.h rfx_renderer_set_launch_traces; 0 = the default 2^30): larger spans
        render as consecutive launches.  No pixel changes."""
        check(_lib.load().rfx_renderer_set_launch_traces(self._h, int(max_traces)), "set_launch_traces")

    def bounce_form(self) -> int:
        """The last trace launch's bounce kernel (rfx.h rfx_renderer_bounce_form): 0 none, 1 global-memory BVH, 2 the
        LDS-staged BVH."""
        return _lib.load().rfx_renderer_bounce_form(self._h)

    def set_rng_prepass(self, mode: int):
        """The RNG pre-pass of one-device unsplit frames (rfx.h rfx_renderer_set_rng_prepass): 1 the cycle table
        (default), 0 the count and emit kernels of every frame.  No pixel changes."""
        check(_lib.load().rfx_renderer_set_rng_prepass(self._h, int(mode)), "set_rng_prepass")

    def prepass_form(self) -> int:
        """The last launch's pre-pass (rfx.h rfx_renderer_prepass_form): 0 count / emit kernels, 1 the cycle table, 2 the
        one-pass kernel."""
        return _lib.load().rfx_renderer_prepass_form(self._h)

    def kat_rng_seq_prefix(self) -> np.ndarray:
        """The cycle table's prefix of accept counts, rfx_rng_seq_blocks() + 1 words (rfx.h rfx_kat_rng_seq_prefix)."""
        out = np.zeros(_lib.load().rfx_rng_seq_blocks() + 1, np.uint32)
        check(_lib.load().rfx_kat_rng_seq_prefix(self._h, _lib.u32ptr(out)), "rfx_kat_rng_seq_prefix")
        return out

    def kat_rng_seq_legacy(self) -> np.ndarray:
        """The same blocks' accept counts from the per-frame count kernel (rfx.h rfx_kat_rng_seq_legacy)."""
        out = np.zeros(_lib.load().rfx_rng_seq_blocks(), np.uint32)
        check(_lib.load().rfx_kat_rng_seq_legacy(self._h, _lib.u32ptr(out)), "rfx_kat_rng_seq_legacy")
        return out

    def set_tri_accel(self, mode: int):
        """Triangle BVH of non-small scenes (rfx.h rfx_renderer_set_tri_accel): -1 automatic (default), 0 off, 1 on,
        2 on with narrow bundles walking the tree too (A/B).  Takes effect at the next set_scene (which then uploads again).  No pixel changes."""
        check(_lib.load().rfx_renderer_set_tri_accel(self._h, int(mode)), "set_tri_accel")
        self._scene_key = None

    def accel_info(self) -> "_lib.AccelInfo":
        """The uploaded scene's hierarchies (rfx.h rfx_renderer_accel_info)."""
        a = _lib.AccelInfo()
        check(_lib.load().rfx_renderer_accel_info(self._h, C.byref(a)), "accel_info")
        return a

    def set_timing(self, enable):
        """HIP-event timing of the frames (rfx.h rfx_renderer_set_timing): True / 1 every frame, n > 1 every n-th
        frame, False / 0 off."""
        check(_lib.load().rfx_renderer_set_timing(self._h, int(enable)), "set_timing")

    def get_timing(self):
        """(prepass_ms, trace_ms, frames) summed over the frames since the last call (HIP events)."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        check(_lib.load().rfx_renderer_get_timing(self._h, C.byref(a), C.byref(b), C.byref(n)), "get_timing")
        return a.value, b.value, n.value

    # device known-answer entry points (rfx.h rfx_kat_*), on the uploaded scene
    def kat_objects(self, rays: np.ndarray, objects: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        objs = np.ascontiguousarray(objects, np.int32)
        out = np.zeros((rays.shape[0], 15), np.float32)
        check(_lib.load().rfx_kat_objects(self._h, _lib.fptr(rays), objs.ctypes.data_as(C.POINTER(C.c_int32)),
                                          rays.shape[0], _lib.fptr(out)), "rfx_kat_objects")
        return out

    def kat_texels(self, texture: int, inp: np.ndarray) -> np.ndarray:
        inp = np.ascontiguousarray(inp, np.float32)
        out = np.zeros((inp.shape[0], 3), np.float32)
        check(_lib.load().rfx_kat_texels(self._h, int(texture), _lib.fptr(inp), inp.shape[0], _lib.fptr(out)),
              "rfx_kat_texels")
        return out

    def kat_powf(self, xy: np.ndarray) -> np.ndarray:
        xy = np.ascontiguousarray(xy, np.float32)
        out = np.zeros(xy.shape[0], np.float32)
        check(_lib.load().rfx_kat_powf(self._h, _lib.fptr(xy), xy.shape[0], _lib.fptr(out)), "rfx_kat_powf")
        return out

    def kat_far_light(self, points: np.ndarray) -> np.ndarray:
        """(n, 8) float32: the general form's light terms at each point, NaN rows where the far form differs
        (rfx.h rfx_kat_far_light)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.zeros((pts.shape[0], 8), np.float32)
        check(_lib.load().rfx_kat_far_light(self._h, _lib.fptr(pts), pts.shape[0], _lib.fptr(out)), "rfx_kat_far_light")
        return out

    def kat_powf_cube(self):
        """(mismatches, glibc-path inputs) of the Fresnel cube form vs glibc's algorithm over every float in [0, 1]."""
        counts = (C.c_uint64 * 2)()
        check(_lib.load().rfx_kat_powf_cube(self._h, counts), "rfx_kat_powf_cube")
        return int(counts[0]), int(counts[1])

    def kat_argb(self, rgb: np.ndarray) -> np.ndarray:
        rgb = np.ascontiguousarray(rgb, np.float32)
        out = np.zeros(rgb.shape[0], np.uint32)
        check(_lib.load().rfx_kat_argb(self._h, _lib.fptr(rgb), rgb.shape[0], _lib.u32ptr(out)), "rfx_kat_argb")
        return out

    def rand_dirs(self, seed: int, n: int):
        out = np.zeros((n, 3), np.float32)
        after = C.c_uint32()
        check(_lib.load().rfx_rand_dirs(self._h, seed, n, _lib.fptr(out), C.byref(after)), "rfx_rand_dirs")
        return out, after.value


class Paths:
    """Scene::trace as resumable per-ray states on the device (rfx.h "Paths"), made by Renderer.paths.

    The planes are torch tensors when the rays were one (every call then runs on torch's current stream and gives
    tensors back: int32 for index lists, state and ARGB words), else device arrays of the library's own, read back as
    numpy (uint32 index lists and words).  colour / state / rays / mul / rand / argb read the planes; segments decodes
    the state words.  close() frees a numpy-backed state."""

    PLANES = (("rays", 6, np.float32), ("mul", 3, np.float32), ("colour", 3, np.float32), ("rand", 3, np.float32),
              ("state", 1, np.int32), ("argb", 1, np.uint32))

    def __init__(self, renderer: "Renderer", rays, draw=True):
        self._r, L = renderer, _lib.load()
        is_torch, r, _ = renderer._ray_batch(rays, "paths")
        n = int(r.shape[0])
        if n == 0:
            raise ValueError("paths: at least one ray")
        own = None if isinstance(draw, (bool, int)) else np.ascontiguousarray(draw, np.float32).reshape(-1, 3)
        if own is not None and own.shape[0] != n:
            raise ValueError("paths: one randDir per ray")
        self.n, self._torch, self._dev, self._t = n, is_torch, None, {}
        if is_torch:
            import torch
            self._t["rays"] = r.clone()
            for name, w, dt in self.PLANES[1:]:
                shape = (n, w) if w > 1 else (n,)
                tdt = torch.float32 if dt == np.float32 else torch.int32
                self._t[name] = torch.zeros(shape, dtype=tdt, device=r.device)
            if own is not None:
                self._t["rand"].copy_(torch.from_numpy(own))
            ptr = {k: v.data_ptr() for k, v in self._t.items()}
        else:
            self._dev = Renderer._DeviceArrays(renderer)
            ptr = {"rays": self._dev.put(r).value}
            for name, w, dt in self.PLANES[1:]:
                a = own if name == "rand" and own is not None else np.zeros(n * w, dt)
                ptr[name] = self._dev.put(a).value
        self._planes = _lib.PathPlanes(**{"d_" + k: v for k, v in ptr.items()})
        stream = self._enter()
        check(L.rfx_paths_begin(renderer._h, C.byref(self._planes), n, 1 if own is None and draw else 0,
                                C.c_void_p(stream or None)), "rfx_paths_begin")
        self._leave(stream)

    # torch: the current stream's handle; the legacy default stream has none to pass on, so there a call is fenced on
    # both sides (Renderer.trace_rays).  numpy: the renderer's own stream.
    def _enter(self):
        if not self._torch:
            return None
        import torch
        s = torch.cuda.current_stream(self._t["rays"].device)
        if not s.cuda_stream:
            s.synchronize()
        return s.cuda_stream

    def _leave(self, stream):
        if self._torch and not stream:
            self._r.synchronize()

    def close(self):
        if self._dev is not None:
            self._dev.__exit__()
            self._dev = None
        self._t = {}

    def _plane(self, name):
        if self._torch:
            return self._t[name]
        w, dt = next((w, dt) for k, w, dt in self.PLANES if k == name)
        a = np.empty((self.n, w) if w > 1 else (self.n,), dt)
        return self._dev.get(a, C.c_void_p(getattr(self._planes, "d_" + name)))

    colour = property(lambda self: self._plane("colour"))
    state = property(lambda self: self._plane("state"))
    rays = property(lambda self: self._plane("rays"))
    mul = property(lambda self: self._plane("mul"))
    rand = property(lambda self: self._plane("rand"))
    argb = property(lambda self: self._plane("argb"))

    @property
    def segments(self):
        """Segments run by every path so far (numpy): the state word while live, its complement once ended."""
        s = self.state
        return _lib.path_segments(s.cpu().numpy() if self._torch else s)

    def _index(self, index, what):
        """An index list as (device pointer or None, slots, what keeps it alive)."""
        if index is None:
            return None, self.n, None
        if self._torch:
            import torch
            if isinstance(index, torch.Tensor):
                t = index.to(device=self._t["rays"].device, dtype=torch.int32).reshape(-1).contiguous()
            else:
                a = np.ascontiguousarray(index).astype(np.uint32).view(np.int32).reshape(-1)
                t = torch.from_numpy(a).to(self._t["rays"].device)
            if t.numel() == 0:
                raise ValueError(f"{what}: an empty index list")
            return t.data_ptr(), int(t.numel()), t
        a = np.ascontiguousarray(index).astype(np.uint32).reshape(-1)
        if a.size == 0:
            raise ValueError(f"{what}: an empty index list")
        return self._dev.put(a).value, int(a.size), None

    def _words(self, count):
        """(device pointer, holder) of `count` uint32 of scratch."""
        if self._torch:
            import torch
            t = torch.empty(count, dtype=torch.int32, device=self._t["rays"].device)
            return t.data_ptr(), t
        return self._dev.alloc(4 * count).value, None

    def _free(self, *ptrs):
        """numpy: a call's scratch goes once its results are read (the reads synchronise)."""
        if self._torch:
            return
        gone = {p for p in ptrs if p}
        for p in gone:
            self._dev.L.rfx_device_free(self._r._h, C.c_void_p(p))
        self._dev.ptrs = [q for q in self._dev.ptrs if q.value not in gone]

    def step(self, upto: int, index=None, live: bool = False):
        """rfx_paths_step: run every named live path that has run fewer than ``upto`` segments on to ``upto`` segments
        or to its end.  index: the paths to work on, wave w of the launch taking index[64 w .. 64 w + 63] (None: all,
        in order); an entry >= n is a dead lane.  live=True: return the indices of the named paths that are live after
        the step (in no particular order) -- the next step's index; the count is read back, so this waits for the step."""
        L = _lib.load()
        stream = self._enter()
        d_index, slots, keep = self._index(index, "step")
        d_live = d_count = None
        if live:
            d_live, hold = self._words(slots + 1)  # the list, then its count
            d_count = d_live + 4 * slots
        check(L.rfx_paths_step(self._r._h, C.byref(self._planes), self.n, C.c_void_p(d_index), slots, int(upto),
                               C.c_void_p(d_live), C.c_void_p(d_count), C.c_void_p(stream or None)), "rfx_paths_step")
        self._leave(stream)
        if not live:
            if not self._torch and d_index:
                self._r.synchronize()
                self._free(d_index)
            return None
        if self._torch:
            return hold[:int(hold[slots].item())]
        count = int(self._dev.get(np.empty(1, np.uint32), C.c_void_p(d_count))[0])
        out = self._dev.get(np.empty(count, np.uint32), C.c_void_p(d_live)) if count else np.empty(0, np.uint32)
        self._free(d_index, d_live)
        return out

    def order(self, index=None):
        """rfx_paths_order: the entries of ``index`` (None: every path) stably sorted by the coherent-order key of the
        paths' current rays, entries >= n last -- the index of a step whose waves should hold like rays."""
        L = _lib.load()
        stream = self._enter()
        d_index, slots, keep = self._index(index, "order")
        d_order, hold = self._words(slots)
        check(L.rfx_paths_order(self._r._h, C.byref(self._planes), self.n, C.c_void_p(d_index), slots,
                                C.c_void_p(d_order), C.c_void_p(stream or None)), "rfx_paths_order")
        self._leave(stream)
        if self._torch:
            return hold
        out = self._dev.get(np.empty(slots, np.uint32), C.c_void_p(d_order))
        self._free(d_index, d_order)
        return out


def make_frame(camera: Camera, W: int, H: int, reflect_num: int, sample_num: int = 1, additive: bool = False,
               additive_counter: int = 0, row_block: int = 0, rank: int = 0, nranks: int = 1,
               pixel_begin: int = 0, pixel_end: int = 0) -> _lib.Frame:
    f = _lib.Frame()
    f.eye[:] = list(camera.eye)
    f.view[:] = list(camera.view)
    f.fov = camera.fov
    f.width, f.height = W, H
    f.reflect_num, f.sample_num = reflect_num, sample_num
    f.additive, f.additive_counter = int(bool(additive)), additive_counter
    f.row_block, f.rank, f.nranks = row_block, rank, nranks
    f.pixel_begin, f.pixel_end = pixel_begin, pixel_end
    return f


class Render:
    """Render (Render.h:7-42) over the GPU renderer."""

    def __init__(self, exePath: str = "", device: int = 0, sphere_seed: int = DEFAULT_SPHERE_SEED,
                 jitter_seed: int = DEFAULT_JITTER_SEED, load_default_scene: bool = True):
        self._r = Renderer(device, sphere_seed, jitter_seed)
        self.imageWidth = 0
        self.imageHeight = 0
        self.additiveCounter = 0
        self.inProgress = False
        self._curx = 0
        self._cury = 0
        self._d_img = None
        self._cap = 0
        self._host = None
        self._host_valid = False
        self.camera = Camera()
        self.scene = Scene()
        self._refl = 0
        self._ss = 0
        self._additive = False
        if load_default_scene:
            self.loadScene(exePath)

    def loadScene(self, exePath: str):
        """Render::loadScene (Render.cpp:25-55)."""
        from . import scenes
        sky = os.path.join(exePath, "./textures/skybox.tga")
        plane = os.path.join(exePath, "./textures/himiya.tga")
        self.camera = Camera(Vector3(*scenes.DEFAULT_CAMERA[0]), Vector3(*scenes.DEFAULT_CAMERA[1]), scenes.DEFAULT_CAMERA[2])
        self.scene = Scene(Color(0.95, 0.95, 1.0), 0.15)
        self.scene.setSkyboxTexture(sky)
        self.scene.addLight(Vector3(11.8e9, 4.26e9, 3.08e9), 3.48e8, Color(1.0, 1.0, 0.95), 0.85)
        for (c, r, mt, rgb, refl) in [
            ((-1.25, 1.5, -0.25), 1.5, METAL, (1.0, 1.0, 1.0), 1.0), ((0.15, 1.0, 1.75), 1.0, METAL, (1.0, 1.0, 1.0), 0.95),
            ((-3.0, 0.6, -3.0), 0.6, DIELECTRIC, (1.0, 1.0, 1.0), 0.0), ((-0.5, 0.5, -2.5), 0.5, DIELECTRIC, (0.5, 1.0, 0.15), 0.75),
            ((1.0, 0.4, -1.5), 0.4, DIELECTRIC, (0.0, 0.5, 1.0), 1.0), ((1.8, 0.4, 0.1), 0.4, METAL, (1.0, 0.65, 0.45), 1.0),
            ((1.7, 0.5, 1.9), 0.5, METAL, (1.0, 0.90, 0.60), 0.75), ((0.6, 0.6, 4.2), 0.6, METAL, (0.9, 0.9, 0.9), 0.0)]:
            self.scene.addSphere(Vector3(*c), r, Material(mt, Color(*rgb), refl, 0.0))
        tex = self.scene.addTexture(plane)
        tr1 = self.scene.addTriangle(Vector3(-14.0, 0.0, -10.0), Vector3(-14.0, 0.0, 10.0), Vector3(14.0, 0.0, -10.0),
                                     Material(DIELECTRIC, Color(1.0, 1.0, 1.0), 0.95, 0.0))
        tr1.setTexture(tex, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0)
        tr2 = self.scene.addTriangle(Vector3(-14.0, 0.0, 10.0), Vector3(14.0, 0.0, 10.0), Vector3(14.0, 0.0, -10.0),
                                     Material(DIELECTRIC, Color(1.0, 1.0, 1.0), 0.95, 0.0))
        tr2.setTexture(tex, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0)

    # -- image buffer ------------------------------------------------------
    def setImageSize(self, width: int, height: int):                      # Render.cpp:57-80
        if width <= 0 or height <= 0:
            return
        L = _lib.load()
        n = width * height * 3 * 4
        if n > self._cap:
            if self._d_img:
                check(L.rfx_device_free(self._r._h, self._d_img), "device_free")
                self._d_img = None
            p = C.c_void_p()
            check(L.rfx_device_alloc(self._r._h, n, C.byref(p)), "device_alloc")
            self._d_img, self._cap = p, n
        zeros = np.zeros(width * height * 3, np.float32)
        check(L.rfx_memcpy_h2d(self._r._h, self._d_img, zeros.ctypes.data_as(C.c_void_p), n), "memcpy_h2d")
        self.imageWidth, self.imageHeight = width, height
        self.additiveCounter = 0
        self.inProgress = False
        self._curx = self._cury = 0
        self._host_valid = False

    def _image(self) -> np.ndarray:
        if not self._host_valid:
            n = self.imageWidth * self.imageHeight
            self._host = np.empty((self.imageHeight, self.imageWidth, 3), np.float32)
            check(_lib.load().rfx_memcpy_d2h(self._r._h, self._host.ctypes.data_as(C.c_void_p), self._d_img, n * 12), "memcpy_d2h")
            self._host_valid = True
        return self._host

    @property
    def image(self) -> np.ndarray:
        """The float framebuffer (std::vector<Color> image, Render.h:10), row 0 = bottom."""
        return self._image()

    def imagePixel(self, x: int, y: int) -> Color:                       # Render.cpp:103-114
        if x < 0 or y < 0:
            return Color(0, 0, 0)
        c = self._image()[y, x]
        if self.additiveCounter > 1:
            k = np.float32(self.additiveCounter)
            return Color(*(c / k).astype(np.float32))
        return Color(*c)

    def imagePixels(self) -> np.ndarray:
        """imagePixel for every pixel at once."""
        img = self._image()
        if self.additiveCounter > 1:
            return (img / np.float32(self.additiveCounter)).astype(np.float32)
        return img.copy()

    def copyImage(self) -> np.ndarray:                                   # Render.cpp:82-101
        """ARGB (h, w) uint32 of the stored (not averaged) image, as Render::copyImage writes a Texture."""
        img = np.ascontiguousarray(self._image())
        out = np.empty((self.imageHeight, self.imageWidth), np.uint32)
        _lib.load().rfx_argb_from_rgb(_lib.fptr(img), img.shape[0] * img.shape[1], _lib.u32ptr(out))
        return out

    # -- rendering ---------------------------------------------------------
    def renderBegin(self, reflectNum: int, sampleNum: int, additive: bool):  # Render.cpp:116-134
        if reflectNum <= 0 or sampleNum == 0:
            raise ValueError("renderBegin: reflectNum > 0 and sampleNum != 0 required (reference asserts)")
        self._refl, self._ss, self._additive = reflectNum, sampleNum, bool(additive)
        self.inProgress = True
        self._curx = self._cury = 0
        self._view = list(self.camera.view)
        self._eye = Vector3(*self.camera.eye)
        self.additiveCounter = self.additiveCounter + 1 if additive else 0

    def renderNext(self, pixels: int) -> bool:                              # Render.cpp:136-215
        W, H = self.imageWidth, self.imageHeight
        if not pixels or not self.inProgress or self._curx >= W or self._cury >= H:
            return False
        p0 = self._cury * W + self._curx
        p1 = min(p0 + pixels, W * H)
        cam = Camera.__new__(Camera)
        cam.eye, cam.view, cam.fov = self._eye, self._view, self.camera.fov
        self._r.set_scene(self.scene)
        f = make_frame(cam, W, H, self._refl, self._ss, self._additive, self.additiveCounter,
                       pixel_begin=p0, pixel_end=p1)
        self._r.render_frame(f, self._d_img.value)
        self._host_valid = False
        self._curx, self._cury = p1 % W, p1 // W
        if p1 == W * H:
            self._curx, self._cury = 0, H
            self.inProgress = False
        return self.inProgress

    def renderAll(self, reflectNum: int, sampleNum: int, additive: bool):   # Render.cpp:217-221 (sic)
        self.renderBegin(reflectNum, sampleNum, additive)
        self.renderNext(self.imageHeight)

    def getRenderProgress(self) -> float:                                   # Render.cpp:223-226
        W, H = self.imageWidth, self.imageHeight
        return float(np.float32(self._curx + self._cury * W) * np.float32(100.0) / np.float32(W) / np.float32(H))

    def traceRays(self, origins, rays, reflNumber: int):
        """Scene::trace(origin, ray, reflNumber) (Scene.h:39) for every row of ``origins`` and ``rays`` ((n, 3) each, or
        one origin for all), in order, on this object's scene: the (n, 3) colours, numpy in, numpy out; torch device
        tensors in, a tensor out (Renderer.trace_rays).  The sphere stream moves n draws on, as after the reference's
        n calls."""
        if reflNumber <= 0:
            raise ValueError("traceRays: reflNumber > 0 required (Scene::trace asserts)")
        self._r.set_scene(self.scene)
        try:
            import torch
            is_torch = isinstance(rays, torch.Tensor)
        except ImportError:
            is_torch = False
        if is_torch:
            d = rays.to(torch.float32).reshape(-1, 3)
            o = torch.as_tensor(origins, dtype=torch.float32, device=d.device).reshape(-1, 3).expand(d.shape[0], 3)
            return self._r.trace_rays(torch.cat([o, d], dim=1), reflNumber)
        d = np.asarray(rays, np.float32).reshape(-1, 3)
        o = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), d.shape)
        return self._r.trace_rays(np.concatenate([o, d], axis=1), reflNumber)

    def pick(self, x: int, y: int, layer: int = 0):
        """What lies under pixel (x, y) of the current camera and image size (row 0 = bottom): (object index as the add
        call returned it, or -1 for the sky; its distance from the eye, |ray t| -- FLT_MAX for the sky).  The ray is cameras.pinhole_ray's, the pixel loop's own (Render.cpp:146-156).
        layer: what lies behind that many hits (Renderer.query_layers); (-1, FLT_MAX) once the ray has run out."""
        from . import cameras
        W, H = self.imageWidth, self.imageHeight
        if not (0 <= x < W and 0 <= y < H):
            raise ValueError("pick: the pixel lies outside the image")
        self._r.set_scene(self.scene)
        ray = cameras.pinhole_ray(tuple(self.camera.eye), self.camera.view, self.camera.fov, W, H, x, y)
        if layer < 0:
            raise ValueError("pick: layer >= 0 required")
        if layer:
            out = self._r.query_layers(ray[None, :], layer + 1, want=("object", "distance"))[layer]
        else:
            out = self._r.query_hits(ray[None, :], want=("object", "distance"))
        return int(out["object"][0]), float(out["distance"][0])

    def getRng(self):
        return self._r.get_rng()

    def synchronize(self):
        self._r.synchronize()

    def close(self):
        L = _lib._lib
        if getattr(self, "_d_img", None) and L is not None and self._r._h:
            L.rfx_device_free(self._r._h, self._d_img)
            self._d_img = None
        self._r.close()
