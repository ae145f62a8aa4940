"""Shared by tests/test_wide_tree_check.py (CPU) and tests/test_gpu_wide_structure.py: running
tools/micro/wide_tree_check (tests/cpp/wide_tree_check.cpp, built by the package Makefile) on a wide
tree given as arrays, and a numpy reading of the node records (layout: host/pt_wide8.cpp) for the
tests that damage a tree on purpose."""
import math
import os
import re
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(REPO, "tools", "micro", "wide_tree_check")
NODE_DWORDS = 20
EMIN_SHIFT = 18           # pt::kW8EminShift
HOST_CAPACITY = 1 << 24   # the host build has no capacity of its own: the encoding's limit


def checker():
    assert os.path.exists(CHECK), "tools/micro/wide_tree_check not built (make -C path-tracer-cuda-opengl_amd)"
    return CHECK


def write_objects(directory, objs, name="objects.bin"):
    path = os.path.join(str(directory), name)
    np.ascontiguousarray(objs).tofile(path)
    return path


def build_host(directory, objects_path):
    """pt::buildWide8 on the objects, through the checker's build mode: (nodes, prims, depth, slots)."""
    nb, pb = os.path.join(str(directory), "host_nodes.bin"), os.path.join(str(directory), "host_prims.bin")
    r = subprocess.run([checker(), "build", objects_path, nb, pb], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"depth (\d+) slots (\d+)", r.stdout.strip())
    assert m, r.stdout
    nodes = np.fromfile(nb, np.uint32).reshape(-1, NODE_DWORDS)
    prims = np.fromfile(pb, np.uint32).reshape(-1, 12)
    assert len(nodes) == int(m.group(2))
    return nodes, prims, int(m.group(1)), int(m.group(2))


def run_check(directory, objects_path, nodes, prims, depth, slots, capacity):
    """The checker on one tree: (return code, stdout + stderr)."""
    nb, pb = os.path.join(str(directory), "nodes.bin"), os.path.join(str(directory), "prims.bin")
    np.ascontiguousarray(nodes, np.uint32).tofile(nb)
    np.ascontiguousarray(prims, np.uint32).tofile(pb)
    r = subprocess.run([checker(), "check", objects_path, nb, pb, str(depth), str(slots), str(capacity)],
                       capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


def failed_checks(output):
    """The names of the checks a run reported."""
    return set(re.findall(r"^CHECK FAILED: (.*?) \(at ", output, flags=re.M))


# ------------------------------------------------------------------ reading node records in numpy
def meta_of(R, j):
    return (int(R[6 + (j >> 2)]) >> (8 * (j & 3))) & 0xff


def is_internal(meta):
    return (meta & 0x18) == 0x18


def leaf_count(meta):
    return {1: 1, 3: 2, 7: 3}[meta >> 5]


def plane_dword(axis, j, high):
    """(dword, shift) of child j's low / high plane byte on `axis`."""
    return 8 + 4 * axis + (2 if high else 0) + (j >> 2), 8 * (j & 3)


def decode_planes(R, j):
    """Child j's planes, exact in float64: (lo[3], hi[3], quantum[3])."""
    lo, hi, q = [], [], []
    for a in range(3):
        s = math.ldexp(1.0, ((int(R[3]) >> (8 * a)) & 0xff) - 127)
        p = float(np.array([R[a]], np.uint32).view(np.float32)[0])
        d, sh = plane_dword(a, j, False)
        lo.append(p + ((int(R[d]) >> sh) & 0xff) * s)
        d, sh = plane_dword(a, j, True)
        hi.append(p + ((int(R[d]) >> sh) & 0xff) * s)
        q.append(s)
    return lo, hi, q


def prim_boxes(prims):
    """Exact fp32 boxes of wide-order primitive records, as pt::primRecord takes them: (n, 3) min, max."""
    f = np.ascontiguousarray(prims, np.uint32).view(np.float32).reshape(-1, 12)
    v = np.stack([f[:, 0:3], f[:, 4:7], f[:, 8:11]], 1)
    mn, mx = v.min(1), v.max(1)
    sph = prims[:, 11] != 0
    rr = np.abs(f[:, 4:5])
    mn = np.where(sph[:, None], f[:, 0:3] - rr, mn).astype(np.float32)
    mx = np.where(sph[:, None], f[:, 0:3] + rr, mx).astype(np.float32)
    return mn, mx


def min_quantum(mn, mx):
    """The builders' smallest quantum 2^emin from the exact boxes (pt_wide8.cpp)."""
    lo, hi = mn.astype(np.float64).min(0), mx.astype(np.float64).max(0)
    ext = float(max(np.abs(lo).max(), np.abs(hi).max(), (hi - lo).max()))
    emin = max(-100, math.ceil(math.log2(ext)) - EMIN_SHIFT) if ext > 0 else -100
    return math.ldexp(1.0, emin)


def children(nodes, slot):
    """(j, meta) of the occupied children of a node."""
    return [(j, meta_of(nodes[slot], j)) for j in range(8) if meta_of(nodes[slot], j)]


def prims_below(nodes, slot):
    """Wide-order primitive indices referenced below a node."""
    out = []
    for s in walk_from(nodes, slot):
        for j, m in children(nodes, s):
            if not is_internal(m):
                first = int(nodes[s][5]) + (m & 31)
                out += list(range(first, first + leaf_count(m)))
    return out


def walk_from(nodes, slot):
    """The slots reachable from `slot`, itself first."""
    out, todo = [], [slot]
    while todo:
        s = todo.pop()
        out.append(s)
        for j, m in children(nodes, s):
            if is_internal(m):
                todo.append(int(nodes[s][4]) + (m & 7))
    return out


def set_byte(nodes, slot, dword, shift, value):
    """A copy of `nodes` with one byte replaced."""
    out = nodes.copy()
    w = int(out[slot][dword])
    out[slot][dword] = (w & ~(0xff << shift) & 0xffffffff) | ((value & 0xff) << shift)
    return out
