"""The library's host-only unit (reflaxman_amd/csrc/rfx_scene.cpp: scene builders, TGA files, the hierarchy builders and
SceneBuild, the host half of rfx_renderer_set_scene) under the address and undefined-behaviour sanitizers: compiled by
plain g++ together with a stand-alone checker (tests/native/scene_host_check.cpp) -- no HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflaxman_amd", "csrc")


def test_scene_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scene_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(CSRC, "rfx_scene.cpp"),
                    os.path.join(ROOT, "tests", "native", "scene_host_check.cpp"), "-o", exe, "-lm"], check=True)
    scratch = tmp_path / "files"
    scratch.mkdir()
    r = subprocess.run([exe, str(scratch)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
