#!/usr/bin/env python3
"""Generate tests/golden/tri_accel/*.json from the reference itself (oracle/_ref/refharness): the SHA-256s of the
f32 and ARGB8 frames of the triangle-BVH cases whose geometry the CPU restatement could get wrong in the same way
as the kernels (ill-conditioned, singular and coincident triangles).  Only hashes and parameters are stored.

Test infrastructure only: needs the reference harness (`make -C oracle ref`), never runs on the GPU box.

    python tools/gen_golden_tri.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402
from reflaxman_amd import scenes  # noqa: E402

OUT = os.path.join(gen_golden.GOLDEN, "tri_accel")
# name -> (scene builder, W, H, depth, ss)
CASES = {
    "soup300_degenerate_48x27_d8": (scenes.degenerate_soup_scene, 48, 27, 8, 1),
}


def main():
    if not os.path.exists(gen_golden.HARNESS):
        sys.exit("oracle/_ref/refharness is missing: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    for name, (make, W, H, depth, ss) in CASES.items():
        desc = make()
        with tempfile.TemporaryDirectory() as tmp:
            rgb, argb = gen_golden.render_case(tmp, desc.write(tmp), W, H, depth, ss, False, 1,
                                               gen_golden.DEFAULT_SEED, 0)
        rec = {"scene": desc.name, "W": W, "H": H, "depth": depth, "ss": ss, "additive": False, "frames": 1,
               "sphere_seed": gen_golden.DEFAULT_SEED, "jitter_seed": 0, "triangles": desc.n_triangles,
               "sha_f32": gen_golden.sha(np.ascontiguousarray(rgb).tobytes()),
               "sha_argb": gen_golden.sha(np.ascontiguousarray(argb).tobytes()),
               "generated": "refharness render (the unmodified reference's Render::renderNext)"}
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print(name, rec["sha_f32"][:16], rec["sha_argb"][:16])


if __name__ == "__main__":
    main()
