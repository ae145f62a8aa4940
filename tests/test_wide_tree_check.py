"""CPU tests of the wide-tree structural checker (tests/cpp/wide_tree_checks.hpp through
tools/micro/wide_tree_check): host-built trees (pt::buildWide8) pass, and a copy with one thing
damaged fails under the name of the check that guards it.  The GPU tests
(tests/test_gpu_wide_structure.py) run the same checker on device-built trees, so what is shown here
is that each kind of defect a builder could have is one the checker sees.

Every mutation is chosen by reading the tree in numpy (tests/wide_tree.py), independently of the
checker, and the test asserts that the scene has a place for it instead of skipping."""
import numpy as np
import pytest

import wide_tree as wt
from helpers import deep_stack_scene, random_soup


def soup():
    return random_soup(700, 300, seed=41)[0]


def tripled():
    objs = random_soup(150, 50, seed=42)[0]
    rep = np.concatenate([objs, objs, objs])
    return rep[np.random.default_rng(42).permutation(len(rep))]


SCENES = {
    "soup": soup,
    "tripled": tripled,
    "deep_stack": lambda: deep_stack_scene(64)[0],
    "n1": lambda: random_soup(1, 0, seed=1)[0],
    "n2": lambda: random_soup(1, 1, seed=2)[0],
    "n3": lambda: random_soup(2, 1, seed=3)[0],
    "n9": lambda: random_soup(5, 4, seed=9)[0],
}


class Tree:
    def __init__(self, directory, objs):
        self.dir = directory
        self.objects = wt.write_objects(directory, objs)
        self.nodes, self.prims, self.depth, self.slots = wt.build_host(directory, self.objects)
        self.n = len(objs)

    def check(self, nodes=None, prims=None, depth=None, slots=None, capacity=wt.HOST_CAPACITY):
        return wt.run_check(self.dir, self.objects, self.nodes if nodes is None else nodes,
                            self.prims if prims is None else prims, self.depth if depth is None else depth,
                            self.slots if slots is None else slots, capacity)

    def rejected(self, name, **changed):
        rc, out = self.check(**changed)
        assert rc == 1, out
        assert name in wt.failed_checks(out), out


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Tree(tmp_path_factory.mktemp("wt_" + name), SCENES[name]())
        return made[name]
    return get


@pytest.mark.parametrize("name", list(SCENES))
def test_host_trees_pass(trees, name):
    t = trees(name)
    rc, out = t.check()
    assert rc == 0, out
    assert f"n {t.n} " in out and f" depth {t.depth} " in out and "failures 0" in out
    assert len(t.prims) == t.n and len(t.nodes) == t.slots


def plane_sites(t, high, internal):
    """(slot, j, axis) of children whose low (high) plane, moved inward by one quantum of its node,
    no longer keeps the margin around a primitive below the child: the box touches within one quantum."""
    mn, mx = wt.prim_boxes(t.prims)
    mq = wt.min_quantum(mn, mx)
    sites = []
    for s in wt.walk_from(t.nodes, 0):
        R = t.nodes[s]
        for j, m in wt.children(t.nodes, s):
            if wt.is_internal(m) != internal:
                continue
            if internal:
                below = wt.prims_below(t.nodes, int(R[4]) + (m & 7))
            else:
                first = int(R[5]) + (m & 31)
                below = list(range(first, first + wt.leaf_count(m)))
            lo, hi, q = wt.decode_planes(R, j)
            for a in range(3):
                d, sh = wt.plane_dword(a, j, high)
                byte = (int(R[d]) >> sh) & 0xff
                if high:
                    lost = byte > 0 and hi[a] - q[a] < float(mx[below, a].astype(np.float64).max()) + mq
                else:
                    lost = byte < 255 and lo[a] + q[a] > float(mn[below, a].astype(np.float64).min()) - mq
                if lost:
                    sites.append((s, j, a))
    return sites


@pytest.mark.parametrize("name", ["soup", "tripled", "deep_stack", "n9"])
@pytest.mark.parametrize("internal", [False, True], ids=["leaf_child", "internal_child"])
@pytest.mark.parametrize("high", [False, True], ids=["low_plane_raised", "high_plane_lowered"])
def test_plane_one_step_inside_is_rejected(trees, name, internal, high):
    t = trees(name)
    sites = plane_sites(t, high, internal)
    assert sites, "the scene has no child whose box touches its plane within one quantum"
    # the first, the last and a middle one: different levels of the tree and all three axes over the scenes
    for s, j, a in (sites[0], sites[len(sites) // 2], sites[-1]):
        d, sh = wt.plane_dword(a, j, high)
        byte = (int(t.nodes[s][d]) >> sh) & 0xff
        t.rejected("subtree primitive inside child box" if internal else "leaf inside box",
                   nodes=wt.set_byte(t.nodes, s, d, sh, byte - 1 if high else byte + 1))


def leaves_of(t):
    """(slot, j, meta, first primitive) of every leaf child, in walk order."""
    return [(s, j, m, int(t.nodes[s][5]) + (m & 31)) for s in wt.walk_from(t.nodes, 0)
            for j, m in wt.children(t.nodes, s) if not wt.is_internal(m)]


def meta_site(j):
    return 6 + (j >> 2), 8 * (j & 3)


@pytest.mark.parametrize("name", ["soup", "tripled"])
def test_swapped_records_are_rejected(trees, name):
    """Two primitive records swapped across leaves: each now sits in a box that is not its own."""
    t = trees(name)
    mn, mx = wt.prim_boxes(t.prims)
    centre = 0.5 * (mn.astype(np.float64) + mx)
    far = int(np.argmax(np.linalg.norm(centre - centre[0], axis=1)))
    assert far != 0 and not np.array_equal(t.prims[0, [0, 1, 2]], t.prims[far, [0, 1, 2]])
    prims = t.prims.copy()
    prims[[0, far]] = prims[[far, 0]]
    t.rejected("leaf inside box", prims=prims)
    # a record whose rank word stays in place while its vertices move: the record is no longer its object's
    prims = t.prims.copy()
    prims[0, [0, 1, 2]] = t.prims[far, [0, 1, 2]]
    t.rejected("primitive record is the one of its rank", prims=prims)
    # a rank twice, another one never
    prims = t.prims.copy()
    prims[0] = prims[far]
    t.rejected("every primitive exactly once", prims=prims)


@pytest.mark.parametrize("name", ["soup", "tripled", "deep_stack"])
def test_hole_and_overlap_in_the_leaf_ranges_are_rejected(trees, name):
    t = trees(name)
    multi = [(s, j, m) for s, j, m, _ in leaves_of(t) if wt.leaf_count(m) > 1]
    assert multi, "the scene has no leaf child of several primitives"
    s, j, m = multi[len(multi) // 2]
    d, sh = meta_site(j)
    cleared = ((m >> 5) >> 1) << 5 | (m & 31)   # 7 -> 3, 3 -> 1: the range's last primitive loses its reference
    t.rejected("leaf ranges leave a hole", nodes=wt.set_byte(t.nodes, s, d, sh, cleared))
    # two leaf children of one node with adjacent ranges: the second one's offset moved onto the first
    pairs = []
    for s in wt.walk_from(t.nodes, 0):
        kids = sorted((m & 31, j, m) for j, m in wt.children(t.nodes, s) if not wt.is_internal(m))
        pairs += [(s, kids[i], kids[i + 1]) for i in range(len(kids) - 1)]
    assert pairs, "the scene has no node with two leaf children"
    s, (off0, _, _), (_, j1, m1) = pairs[len(pairs) // 2]
    d, sh = meta_site(j1)
    t.rejected("leaf ranges overlap", nodes=wt.set_byte(t.nodes, s, d, sh, (m1 & 0xe0) | off0))


@pytest.mark.parametrize("name", ["soup", "deep_stack"])
def test_damaged_links_are_rejected(trees, name):
    t = trees(name)
    inner = [(s, j, m) for s in wt.walk_from(t.nodes, 0) for j, m in wt.children(t.nodes, s) if wt.is_internal(m)]
    assert inner and t.slots > 8
    s, j, m = inner[len(inner) // 2]
    d, sh = meta_site(j)
    t.rejected("internal child's slot bits equal its slot", nodes=wt.set_byte(t.nodes, s, d, sh, (m & ~7) | ((m & 7) ^ 1)))
    nodes = t.nodes.copy()
    nodes[s][4] = t.slots   # the child base moved beyond the slots
    t.rejected("child slot in range", nodes=nodes)
    nodes[s][4] = 1 << 24
    t.rejected("child base fits 24 bits", nodes=nodes)
    # a child base moved onto another node's block: those nodes are reached twice
    other = next(int(t.nodes[x][4]) for x, _, _ in inner if int(t.nodes[x][4]) != int(t.nodes[s][4]))
    nodes[s][4] = other
    rc, out = t.check(nodes=nodes)
    assert rc == 1 and wt.failed_checks(out) & {"node reached once", "child slot in range", "leaf ranges overlap"}, out
    t.rejected("exponent byte in range", nodes=wt.set_byte(t.nodes, s, 3, 8, 254))


@pytest.mark.parametrize("name", ["soup", "tripled", "deep_stack"])
def test_misreported_depth_and_slots_are_rejected(trees, name):
    t = trees(name)
    assert t.depth >= 2 and t.slots >= 9
    t.rejected("reported depth equals the walk's", depth=t.depth - 1)
    t.rejected("reported depth equals the walk's", depth=t.depth + 1)
    t.rejected("child block ends within the reported slots", slots=t.slots - 8)
    t.rejected("reported slots within the capacity", capacity=t.slots - 1)
    t.rejected("reported slots within the node array", slots=t.slots + 8)
    rc, out = t.check(capacity=t.slots)
    assert rc == 0, out


def test_usage_and_unreadable_input(trees, tmp_path):
    import subprocess
    t = trees("n9")
    assert subprocess.run([wt.checker()], capture_output=True).returncode == 2
    assert subprocess.run([wt.checker(), "check", str(tmp_path / "missing.bin"), "a", "b", "1", "1", "1"],
                          capture_output=True).returncode == 2
    rc, out = wt.run_check(t.dir, t.objects, t.nodes, t.prims[:-1], t.depth, t.slots, wt.HOST_CAPACITY)
    assert rc == 1 and "primitive array holds n records" in wt.failed_checks(out), out
