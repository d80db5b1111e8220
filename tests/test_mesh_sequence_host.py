"""The moving-mesh sequences, the host side (no device): every script of tests/mesh_sequence.py run through the model
and the host mirror alone, asserting that each script reaches the regime it is there for -- conditions on the inputs,
not on the library -- and that the mirror's trees are trees of the scene's in-tree triangles at every step."""
import numpy as np
import pytest

import mesh_sequence as ms
import recut_helpers as rh


def run(key, ops):
    """the model after every operation: list of (op, expected(), V copy), the state before the first in front"""
    m = ms.Model(key)
    states = [(None, m.expected(), m.V.copy())]
    for op in ops:
        m.apply(op)
        states.append((op, m.expected(), m.V.copy()))
    return m, states


def check_trees(m, states):
    for op, e, _ in states:
        ids = e["leaf_ids"]
        got = ids[ids >= 0]
        assert np.array_equal(np.sort(got), m.tree), op
        assert e["boxes"].shape == (m.dump["nodes"], 2, 6) and e["children"].shape == (m.dump["nodes"], 2)
        slot = ms.slots_of(ids, m.n)
        assert (slot[m.residual] == -1).all() and (slot[m.tree] >= 0).all()


def nan_boxes(e):
    return int(np.isnan(e["boxes"]).any(axis=2).sum())


def touched(before, after):
    return np.flatnonzero((before.view(np.uint32) != after.view(np.uint32)).any(axis=(1, 2)))


def test_partial_updates_reach_a_recut_tree():
    key, ops = ms.partial_updates()
    m, st = run(key, ops)
    check_trees(m, st)
    assert m.n == 384 and len(m.tree) == 384
    assert [o.kind for o in ops] == ["whole", "recut", "range", "indexed", "host_range", "recut", "indexed"]
    assert (ops[2].first, len(ops[2].rows)) == (10, 23) and (ops[3].first, len(ops[3].rows), ops[3].dead) == (40, 9, (44,))
    assert (ops[4].first, len(ops[4].rows)) == (383, 1) and (ops[6].first, len(ops[6].rows), ops[6].dead) == (0, 384, ())
    # after step 1 at least half of the triangles sit in another slot than at set_scene
    moved = (ms.slots_of(st[2][1]["leaf_ids"], m.n) != ms.slots_of(m.dump["leaf_ids"], m.n)).sum()
    assert moved >= m.n // 2, moved
    # each partial update after the re-cut touches triangles of at least three leaves of the re-cut tree (the
    # one-triangle host form: its one leaf) and changes at least one node box
    for k in (3, 4, 5, 7):
        op, e, V = st[k]
        t = touched(st[k - 1][2], V)
        want = len(op.rows) - len(op.dead)
        assert len(t) == want and not np.isin(op.dead, t).any(), (op, len(t))
        leaves = np.unique(ms.slots_of(e["leaf_ids"], m.n)[t] // rh.LEAF)
        assert len(leaves) >= min(3, want), (op, leaves)
        assert e["boxes"].tobytes() != st[k - 1][1]["boxes"].tobytes(), op
        assert np.array_equal(e["leaf_ids"], st[k - 1][1]["leaf_ids"])  # an update moves no triangle
    assert not np.array_equal(st[6][1]["leaf_ids"], st[5][1]["leaf_ids"])  # the second re-cut does


def test_class_changes_reach_their_leaves():
    key, ops, six, three, two = ms.class_changes()
    m, st = run(key, ops)
    check_trees(m, st)
    assert np.isin(six + two, m.tree).all()
    assert [o.kind for o in ops] == ["whole", "recut", "range", "recut", "indexed", "recut"]
    ill = [int(e["ill"].sum()) - len(m.residual) for _, e, _ in st]
    assert ill[0] == 0 and ill[2:] == [6, 3, 3, 5, 5], ill
    G = m.dump["leaves"]
    leaf_of = lambda e, ts: ms.slots_of(e["leaf_ids"], m.n)[ts] // rh.LEAF
    assert (leaf_of(st[2][1], six) >= G - 2).all()  # the six lie in the last leaves
    # the three stay in their leaves when they turn well, and fewer child boxes are all of space
    assert np.array_equal(leaf_of(st[3][1], three), leaf_of(st[2][1], three))
    assert 0 < nan_boxes(st[3][1]) < nan_boxes(st[2][1]), (nan_boxes(st[2][1]), nan_boxes(st[3][1]))
    assert (st[3][1]["ill"][three] == 0).all() and np.array_equal(touched(st[2][2], st[3][2]), three)
    # the re-cut places them
    assert (leaf_of(st[4][1], three) < G - 2).all()
    # two others turn ill under the re-cut tree: NaN spines away from the last leaves
    assert (st[5][1]["ill"][two] == 1).all() and (leaf_of(st[5][1], two) < G - 2).all()
    assert nan_boxes(st[5][1]) > nan_boxes(st[4][1])
    assert (leaf_of(st[6][1], two) >= G - 2).all() and nan_boxes(st[6][1]) < nan_boxes(st[5][1])


@pytest.mark.parametrize("key", ["mesh", "degenerate"])
def test_set_scene_state_is_the_built_tree(key):
    key, ops = ms.set_scene_after_a_recut(key)
    m, st = run(key, ops)
    check_trees(m, st)
    if key == "degenerate":  # here the built tree's depth is not the cut's: a set_scene that kept the cut's would show
        assert (m.dump["depth"], st[2][1]["depth"]) == (8, 7)
    assert [o.kind for o in ops] == ["whole", "recut", "set_scene", "range", "recut"]
    e = st[3][1]
    # the set_scene state's tree is the dump's, bit for bit (the unwidened refit at the scene's own vertices is the dump's
    # boxes; the widened one is what a new renderer holds)
    assert e["leaf_ids"] is m.dump["leaf_ids"] and e["children"] is m.dump["children"] and e["depth"] == m.dump["depth"]
    assert m.scene.tri_bvh_refit(m.V0, widen=False)[0].tobytes() == m.dump["boxes"].tobytes()
    assert e["boxes"].tobytes() == st[0][1]["boxes"].tobytes() and e["mt"].tobytes() == st[0][1]["mt"].tobytes()
    assert st[3][2].tobytes() == m.V0.tobytes()
    assert not np.array_equal(st[2][1]["leaf_ids"], e["leaf_ids"])  # the re-cut before it had changed the membership
    # the update after it is checked against the plain refit, not the cut
    assert np.array_equal(st[4][1]["leaf_ids"], m.dump["leaf_ids"]) and st[4][1]["boxes"].tobytes() != e["boxes"].tobytes()
    assert st[5][1]["depth"] == (m.dump["leaves"] - 1).bit_length()


def test_shared_scratch_script_differs_both_ways():
    key, ops = ms.shared_sort_scratch()
    m, st = run(key, ops)
    check_trees(m, st)
    kinds = [o.kind for o in ops if o.kind in ("order", "recut")]
    assert kinds == ["order", "recut", "order", "recut", "order"]
    ns = [o.n for o in ops if o.kind == "order"]
    assert ns == [3 * ms.T + 5, 65, 3 * ms.T + 5] and ns[1] < len(m.tree) < ns[0]
    cuts = [e["leaf_ids"] for op, e, _ in st if op is not None and op.kind == "recut"]
    assert not np.array_equal(cuts[0], cuts[1])


@pytest.mark.parametrize("seed", ms.WALK_SEEDS)
def test_walks_reach_their_regimes(seed):
    key, ops = ms.walk(seed)
    m, st = run(key, ops)
    check_trees(m, st)
    assert m.n == 324 and len(m.residual) == 14 and len(ops) == 16
    assert all((o.kind == "recut") == (k % 5 == 4) for k, o in enumerate(ops))
    assert sum(o.kind == "recut" for o in ops) >= 2
    assert sum(len(o.dead) for o in ops) >= 1
    hit_residual = class_change = 0
    for k in range(1, len(st)):
        op = st[k][0]
        if op.kind not in ms.UPDATES:
            continue
        t = touched(st[k - 1][2], st[k][2])
        hit_residual += bool(np.isin(t, m.residual).any())
        class_change += bool((st[k][1]["ill"] != st[k - 1][1]["ill"]).any())
    assert hit_residual >= 1 and class_change >= 1, (hit_residual, class_change)
    assert sum(o.check for o in ops) >= 4 and ops[-1].check
