"""The RNG pre-pass from the cycle table (rfx.h rfx_renderer_set_rng_prepass, mode 1) against the per-frame count and
emit kernels (mode 0) and the reference.

The table: per-block accept counts of the LCG's whole cycle of 2^32 triples, against the reference's float accept test
(src/common/Vector3.cpp:182-185) restated in numpy and against the per-frame count kernel.  The frames: bit-equal in
both modes, in one process, at the block and wrap edges of the cycle and across every hand-over of the stream state.
"""
import os

import numpy as np
import pytest

from helpers import GOLDEN, manifest
from reflaxman_amd import _lib, scenes
from test_rng_sequence import A1, C1, M, ORIGIN, affine_pow, jump_triples

pytestmark = pytest.mark.gpu

TPB = 4096  # triples per block of the table
_DESC = {}


def default_scene():
    if "d" not in _DESC:
        _DESC["d"] = scenes.get_scene("default")
    return _DESC["d"]


_TABLE = {}


def table():
    """(prefix, legacy counts) of one renderer, computed once for the module."""
    if not _TABLE:
        from reflaxman_amd.render import Renderer
        rr = Renderer()
        _TABLE["prefix"] = rr.kat_rng_seq_prefix()
        _TABLE["legacy"] = rr.kat_rng_seq_legacy()
        rr.close()
        for a in _TABLE.values():
            a.setflags(write=False)
    return _TABLE["prefix"], _TABLE["legacy"]


def float_block_counts(blocks):
    """Accepted triples of the cycle's blocks by the reference's float test (Vector3.cpp:182-185: x = float(k) /
    (float(0x7FFF) / 2) - 1, rejected when x*x + y*y + z*z > 1), and how many of their threads (runs of 16 triples) hold
    a triple on the integer test's shell."""
    half = np.float32(np.float32(0x7FFF) / np.float32(2))
    x_of = (np.arange(1 << 15, dtype=np.float32) / half - np.float32(1)).astype(np.float32)
    starts = np.array([jump_triples(ORIGIN, TPB * int(b)) for b in blocks], np.uint32)
    tj = [affine_pow(A1, C1, 48 * t) for t in range(256)]
    ta = np.array([a for a, _ in tj], np.uint32)
    tc = np.array([c for _, c in tj], np.uint32)
    with np.errstate(over="ignore"):
        s = (ta[None, :] * starts[:, None] + tc[None, :]).astype(np.uint32)  # block x thread
        cnt = np.zeros(s.shape, np.int64)
        on_shell = np.zeros(s.shape, bool)
        for _ in range(16):
            acc = None
            n = np.zeros(s.shape, np.int64)
            for _d in range(3):
                s = np.uint32(A1) * s + np.uint32(C1)
                kk = ((s >> 16) & 0x7FFF).astype(np.int64)
                x = x_of[kk]
                acc = (x * x).astype(np.float32) if acc is None else (acc + x * x).astype(np.float32)
                n += (2 * kk - 32767) ** 2
            cnt += ~(acc > np.float32(1))
            on_shell |= np.abs(n - 32767 * 32767) <= 1024
    return cnt.sum(1), int(on_shell.sum())


def test_table_blocks_equal_the_float_test():
    prefix, _ = table()
    nb = _lib.load().rfx_rng_seq_blocks()
    assert nb * TPB == M and prefix.shape[0] == nb + 1 and prefix[0] == 0
    rng = np.random.default_rng(7)
    blocks = np.sort(np.concatenate([[0, nb - 1], 1 + rng.choice(nb - 2, 1022, replace=False)]))
    assert blocks.shape[0] == 1024 and np.unique(blocks).shape[0] == 1024
    want, shell_threads = float_block_counts(blocks)
    got = prefix[blocks + 1].astype(np.int64) - prefix[blocks].astype(np.int64)
    # about 2.4e-5 of the threads hold a triple on the shell (its lattice points over 2^45, times 16): 6 expected among
    # these 262,144, and at least one needed for the float redo to have decided a count here
    assert shell_threads >= 1
    assert np.array_equal(got, want)
    # the cycle's total: about pi / 6 of 2^32 triples
    assert abs(int(prefix[nb]) / 2.0 ** 32 - np.pi / 6) < 1e-4


def test_table_equals_the_count_kernel():
    prefix, legacy = table()
    assert np.array_equal(np.diff(prefix.astype(np.int64)), legacy.astype(np.int64))


def render_steps(mode, W, H, steps, seed=1350490027, launch_traces=None):
    """Frames through the Python mirror of Render with the pre-pass `mode`; a step is (depth, ss, additive, chunks) or
    ("set_rng", sphere, jitter) or ("rewind",).  Returns per frame (f32 bytes, ARGB bytes, prepass form)."""
    from reflaxman_amd.render import Render, build_scene
    r = Render(sphere_seed=seed, jitter_seed=0, load_default_scene=False)
    r.scene, r.camera = build_scene(default_scene())
    r._r.set_rng_prepass(mode)
    if launch_traces is not None:
        r._r.set_launch_traces(launch_traces)
    r.setImageSize(W, H)
    out = []
    for st in steps:
        if st[0] == "set_rng":
            r._r.set_rng(st[1], st[2])
            continue
        if st[0] == "rewind":
            _lib.check(_lib.load().rfx_frame_rng_rewind(r._r._h), "rewind")
            continue
        depth, ss, additive, chunks = st
        r.renderBegin(depth, ss, additive)
        i = 0
        while r.renderNext(chunks[i % len(chunks)] if chunks else W * H):
            i += 1
        form = r._r.prepass_form()
        r.synchronize()
        out.append((r.imagePixels().tobytes(), r.copyImage().tobytes(), form))
    state = r.getRng()
    r.close()
    return out, state


def both_modes(W, H, steps, seed=1350490027, launch_traces=None):
    t, ts = render_steps(1, W, H, steps, seed, launch_traces)
    l, ls = render_steps(0, W, H, steps, seed, launch_traces)
    assert len(t) == len(l)
    for i, (a, b) in enumerate(zip(t, l)):
        assert a[0] == b[0], f"frame {i}: f32 differs"
        assert a[1] == b[1], f"frame {i}: ARGB8 differs"
        assert b[2] != 1, f"frame {i}: mode 0 took the table"
    assert ts == ls  # both random streams end in the same state
    return t


PLAIN = (4, 1, False, None)


def test_frames_both_paths_one_process():
    t = both_modes(160, 120, [PLAIN] * 4)
    assert all(f[2] == 1 for f in t)  # the table path ran
    assert manifest()["cases"]["render_default_160x120_d4"]["sphere_seed"] == 1350490027
    g = np.load(os.path.join(GOLDEN, "render_default_160x120_d4.npz"))
    assert t[0][0] == np.ascontiguousarray(g["rgb"]).tobytes()
    assert t[0][1] == np.ascontiguousarray(g["argb"]).tobytes()


EDGES = {
    "block_boundary": TPB * 12345,
    "last_thread": TPB * 777 + TPB - 6,
    "across_wrap": M - 5000,
    "last_triple": M - 1,
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_block_and_wrap_edges(edge):
    k = EDGES[edge]
    seed = jump_triples(ORIGIN, k)
    assert _lib.load().rfx_rng_triple_index(seed) == k
    for W, H, depth in ((7, 3, 8), (160, 120, 4)):
        t = both_modes(W, H, [(depth, 1, False, None)] * 2, seed)
        assert all(f[2] == 1 for f in t)


def test_one_trace_frame():
    for seed in (1350490027, jump_triples(ORIGIN, M - 1), jump_triples(ORIGIN, TPB * 5)):
        t = both_modes(1, 1, [(8, 1, False, None)] * 3, seed)
        assert all(f[2] == 1 for f in t)


@pytest.mark.parametrize("steps", [
    [PLAIN, ("set_rng", 987654321, 5), PLAIN],
    [PLAIN, (4, 1, False, [7, 1000, 13]), PLAIN],
    [PLAIN, (4, 2, False, None), (4, 1, True, None), PLAIN],
    [PLAIN, ("rewind",), PLAIN],
], ids=["set_rng", "chunked", "ssaa_additive", "rewind"])
def test_state_hand_over(steps):
    t = both_modes(160, 120, steps)
    assert t[0][2] == 1 and t[-1][2] == 1


def test_split_spans():
    """An 8x6 frame of 16x16 samples under a launch limit of one pixel row (six spans on two streams, each starting
    from the place in the cycle the span before it wrote), then a plain frame, from a start that crosses the wrap."""
    steps = [(4, 16, False, None), (4, 1, False, None), (4, 16, True, None)]
    for seed in (1350490027, jump_triples(ORIGIN, M - 3000)):
        t = both_modes(8, 6, steps, seed, launch_traces=16 * 16 * 8)
        assert all(f[2] == 1 for f in t)
    g = np.load(os.path.join(GOLDEN, "render_default_160x120_d4.npz"))
    t = both_modes(160, 120, [PLAIN], launch_traces=100)  # spans that start mid-row
    assert t[0][2] == 1 and t[0][0] == np.ascontiguousarray(g["rgb"]).tobytes()
