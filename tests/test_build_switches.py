"""A tools/ab.py variant cannot silently be a second `base`, and a switch has one default.

Every compile-time switch of librfx.so is declared in reflaxman_amd/csrc/rfx_config.h: a value switch by its one
`#ifndef NAME / #define NAME default / #endif`, a switch that takes another's value when unset and the presence flags
by a line of the header's two commented lists.  A variant that passes a name no source reads builds `base` again and
the A/B reports session noise as a result, so every define of tools/ab.py's VARIANTS must be declared there; a second
default elsewhere would let host and device units disagree, so there is none; and the experiments whose code was removed
stay removed.  Text only: neither the HIP runtime nor the library is loaded.
"""
import ast
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflaxman_amd", "csrc")
CONFIG = os.path.join(CSRC, "rfx_config.h")

# the flags rfx_bounce.h defines itself unless RFX_NO_LAUNDER is given (a variant may also pass either alone): the one
# exception to "no #define of a switch outside rfx_config.h"
DERIVED_FROM_NO_LAUNDER = {"RFX_LAUNDER_SCENE", "RFX_LAUNDER_PARAMS"}

REMOVED = ["RFX_HALF_BUNDLES", "RFX_SSAA_LDS_STATE", "RFX_BVH_TLIM", "RFX_BVH_PREWIDE", "RFX_BVH_FMA", "RFX_DIV_SEL",
           "RFX_PRIM_LARGE", "prim_cull_large_kernel"]


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def declared():
    """(value switches with a default in the header, names its commented lists declare)."""
    text = read(CONFIG)
    defaults = set(re.findall(r"^#ifndef (RFX_\w+)\n#define \1\b", text, re.M))
    listed = set(re.findall(r"^//   (RFX_\w+)\s", text, re.M))
    return defaults, listed


def variants():
    tree = ast.parse(read(os.path.join(ROOT, "tools", "ab.py")))
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "VARIANTS" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("tools/ab.py: no VARIANTS")


def test_header_declares_switches_and_flags():
    defaults, listed = declared()
    assert len(defaults) > 30 and not defaults & listed
    assert {"RFX_NO_LAUNDER", "RFX_DEBUG_PROF", "RFX_DEBUG_SEGS", "RFX_DEBUG_WAVES"} | DERIVED_FROM_NO_LAUNDER <= listed
    # every #ifndef of the header is a default of the form the other tests look for
    assert set(re.findall(r"^#ifndef (RFX_\w+)", read(CONFIG), re.M)) == defaults


def test_every_variant_define_is_a_declared_switch():
    defaults, listed = declared()
    v = variants()
    assert "base" in v and v["base"] == []
    unknown = {(name, d) for name, defs in v.items() for d in defs
               if not d.startswith("-") and d.split("=")[0] not in defaults | listed}  # "-...": a compiler flag
    assert not unknown, unknown


def test_no_switch_is_defined_outside_the_header():
    defaults, listed = declared()
    names = (defaults | listed) - DERIVED_FROM_NO_LAUNDER
    second = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isdir(path) or path == CONFIG:
            continue
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", read(path), re.M):
            if m.group(1) in names:
                second.append((os.path.basename(path), m.group(1)))
    # a switch that takes another's value when unset has its (only) default where that value is in scope: at trace_kernel
    assert second == [("rfx_trace.h", "RFX_WAVES_PER_EU_LARGE")], second
    # and the exception is what it says: rfx_bounce.h (the bounce loop, which reads the laundered arguments) derives both
    # flags under #ifndef RFX_NO_LAUNDER, nothing else does
    bounce = read(os.path.join(CSRC, "rfx_bounce.h"))
    assert "#ifndef RFX_NO_LAUNDER\n#define RFX_LAUNDER_SCENE\n#define RFX_LAUNDER_PARAMS\n#endif\n" in bounce
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isdir(path):
            n = len(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(?:%s)\b" % "|".join(DERIVED_FROM_NO_LAUNDER), read(path), re.M))
            assert n == (2 if os.path.basename(path) == "rfx_bounce.h" else 0), path


@pytest.mark.parametrize("name", REMOVED)
def test_removed_experiments_stay_removed(name):
    files = [p for pat in ("reflaxman_amd/**/*", "tools/*.py", "tests/**/*", "include/**/*")
             for p in glob.glob(os.path.join(ROOT, pat), recursive=True)
             if os.path.isfile(p) and "__pycache__" not in p and os.path.abspath(p) != os.path.abspath(__file__)
             and not p.startswith(os.path.join(ROOT, "reflaxman_amd", "lib") + os.sep)]  # build products are not sources
    assert len(files) > 100
    allowed = "RFX_BUILD_PRIM_LARGE" if name == "RFX_PRIM_LARGE" else None  # the reserved ABI bit of include/rfx.h
    hits = []
    for p in files:
        try:
            text = read(p)
        except UnicodeDecodeError:  # binary test vectors
            continue
        if allowed:
            text = text.replace(allowed, "")
        if name in text:
            hits.append(os.path.relpath(p, ROOT))
    assert not hits, hits
