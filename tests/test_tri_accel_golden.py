"""The CPU restatement against the reference's own frames of the triangle-BVH cases (tests/golden/tri_accel, written
by tools/gen_golden_tri.py from the unmodified reference): the GPU tests of tests/test_gpu_tri_accel.py compare with
the restatement, so it must itself be the reference on slivers, zero-area and coincident triangles."""
import glob
import json
import os

import pytest

from helpers import GOLDEN, sha
from reflaxman_amd import scenes

CASES = sorted(glob.glob(os.path.join(GOLDEN, "tri_accel", "*.json")))
BUILDERS = {"soup300_degenerate": scenes.degenerate_soup_scene}


def test_cases_present():
    assert CASES


@pytest.mark.parametrize("path", CASES, ids=os.path.basename)
def test_oracle_equals_reference_hash(path):
    import oracle as orc
    g = json.load(open(path))
    desc = BUILDERS[g["scene"]]()
    assert desc.n_triangles == g["triangles"]
    o = orc.OracleRender(desc, g["sphere_seed"], g["jitter_seed"])
    o.set_image_size(g["W"], g["H"])
    for _ in range(g["frames"]):
        o.render(g["depth"], g["ss"], g["additive"])
    assert sha(o.image) == g["sha_f32"]
    assert sha(o.argb()) == g["sha_argb"]
