"""Record the reference's own outputs -> tests/golden/reference_fixtures.npz (inputs next to outputs).

Runs the reference programs of oracle/_ref/ (`make -C oracle ref`; oracle/refharness.py) on the
cases of tests/reference_cases.py that go beyond tests/golden/oracle_fixtures.npz:

  lbvh_{soup,dup}_{n}_*   objects -> sorted keys and buildBVH's nodes (origin-seeded boxes), n = 1 .. 1000
  deg_{scene}_*           degenerate and ordinary rays (every 8th ray of each class of
                          tests/degenerate_rays.py) -> hitBvh's records, interval [0.001, inf); plus
                          `lib_hits`: the same records under include/pt.h's one change (a NaN candidate
                          is no hit), which is what the kernels are held to -- see lib_rule() below
  sc_*                    the constructed Material::scatter edges -> ok, ray, attenuation, draws used,
                          under both draw orders (sc_*_xyz from the clang++ program, sc_*_zyx from g++)
  fr_{frame}_*            four small frames (rtiow, triangle_world, cornell, the L2 soup) -> fp32 images
                          and the XORWOW states after every launch (L2 launches twice)
  draw_order              "xyz": the order the frames (and the kernels) draw vec3(u, u, u)'s coordinates
                          in -- the clang++ program's; pixel 0 of a frame is the reference's own and is
                          the one pixel no comparison uses (main.cu:286)

Data only.  tests/test_reference_fixtures.py checks the oracle (and, where built, the reference
programs again) against the file; tests/test_gpu_reference_fixtures.py checks the kernels.

usage: python tools/make_reference_fixtures.py        (CPU; a few seconds)
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "path-tracer-cuda-opengl_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import oracle  # noqa: E402
import ptamd  # noqa: E402
import reference_cases as rc  # noqa: E402
import refharness as rh  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "reference_fixtures.npz")
DEG_STRIDE = 8
FRAMES = ("rtiow", "triangle_world", "cornell", "l2")
MISS = np.zeros(1, rh.HIT_DTYPE)
MISS["obj"] = MISS["mat"] = -1


def canon(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same(a, b):
    return np.array_equal(canon(a), canon(b))


def lib_rule(ref_hits, objs, rays):
    """The records the library is held to, from the reference's: a record whose t is NaN becomes the
    miss record {0, -1, -1, 0, 0...} (pt.h's one stated change).  A ray whose traversal accepted a NaN
    candidate on the way and ended on a finite one keeps, in the reference, whichever candidate came
    last; the library's rule gives it the closest finite candidate instead, which the reference
    cannot tell us.  Those rays take the oracle's nan_miss=True record (the oracle being pinned to
    the reference bit for bit on these very rays with nan_miss=False); `via_nan` marks them."""
    nodes = oracle.build_lbvh(objs, oracle.morton_keys(objs), tight=False)
    plain, _ = oracle.trace(objs, nodes, rays, nan_miss=False)
    ruled, _ = oracle.trace(objs, nodes, rays, nan_miss=True)
    for f in ("hit", "mat", "front_face"):
        assert np.array_equal(plain[f], ref_hits[f]), f
    h = ref_hits["hit"] == 1
    assert all(same(plain[f][h], ref_hits[f][h]) for f in ("t", "p", "n"))
    out = ref_hits.copy()
    out["obj"] = plain["obj"]            # hit_record has no object id: the (pinned) oracle's
    nan_t = h & np.isnan(ref_hits["t"])
    out[nan_t] = MISS[0]
    differs = np.zeros(len(out), bool)
    for f in ("hit", "obj", "mat", "front_face"):
        differs |= out[f] != ruled[f]
    for f in ("t", "p", "n"):
        differs |= (canon(out[f]) != canon(ruled[f])).reshape(len(out), -1).any(axis=1)
    out[differs] = ruled[differs]
    return out, differs


def main():
    if not rh.available():
        sys.exit("oracle/_ref/ holds no reference programs: run `make -C oracle ref` with the reference tree present")
    fx = {"draw_order": np.frombuffer(b"xyz", np.uint8)}

    for kind in rc.LBVH_KINDS:
        for n in rc.LBVH_SIZES:
            objs = rc.lbvh_objects(kind, n)
            keys, nodes = rh.build_lbvh("clang", objs)
            k2, n2 = rh.build_lbvh("gxx", objs)
            assert np.array_equal(keys, k2) and nodes.tobytes() == n2.tobytes()
            fx[f"lbvh_{kind}_{n}_objects"], fx[f"lbvh_{kind}_{n}_keys"], fx[f"lbvh_{kind}_{n}_nodes"] = objs, keys, nodes
    mats = np.zeros(4, oracle.MATERIAL_DTYPE)
    mats["type"] = 1
    mats["albedo"] = 0.5
    fx["lbvh_materials"] = mats

    for name, objs in rc.degenerate_scenes().items():
        rays, where = rc.degenerate_batch(objs, DEG_STRIDE)
        hits = rh.trace("clang", objs, rays)
        h2 = rh.trace("gxx", objs, rays)
        assert all(np.array_equal(hits[f], h2[f]) for f in ("hit", "mat", "front_face"))
        assert all(same(hits[f][hits["hit"] == 1], h2[f][hits["hit"] == 1]) for f in ("t", "p", "n"))
        for f in ("t", "p", "n"):   # one NaN pattern in the file, whatever the host's
            hits[f] = canon(hits[f]).view(np.float32)
        lib, via = lib_rule(hits, objs, rays)
        fx[f"deg_{name}_objects"], fx[f"deg_{name}_rays"] = objs, rays
        fx[f"deg_{name}_hits"], fx[f"deg_{name}_lib_hits"], fx[f"deg_{name}_via_nan"] = hits, lib, via
        print(f"deg {name}: {len(rays)} rays, {int(hits['hit'].sum())} reference hits, "
              f"{int(np.isnan(hits['t'][hits['hit'] == 1]).sum())} with NaN t, {int(via.sum())} via a NaN candidate")
    fx["deg_materials"] = mats
    fx["deg_classes"] = np.array(list(where.keys()))
    fx["deg_class_size"] = np.array([rc.dg.CLASS_RAYS // DEG_STRIDE], np.int32)

    smats, cm, srays, shits, tapes, labels = rc.scatter_edges()
    fx["sc_materials"], fx["sc_case_mat"], fx["sc_case_ray"], fx["sc_case_hit"], fx["sc_tapes"] = smats, cm, srays, shits, tapes
    fx["sc_labels"] = np.array(labels)
    for comp, order in (("clang", "xyz"), ("gxx", "zyx")):
        ok, out, att, used = rh.scatter(comp, smats, cm, srays, shits, tapes)
        fx[f"sc_ok_{order}"], fx[f"sc_used_{order}"] = ok, used
        fx[f"sc_out_{order}"], fx[f"sc_att_{order}"] = canon(out).view(np.float32), canon(att).view(np.float32)

    cases = rc.frame_cases(ptamd, oracle)
    for name in FRAMES:
        c = cases[name]
        rgb, st = rh.render("clang", c["objects"], c["materials"], c["camera"], c["width"], c["height"], c["spp"],
                            c["depth"], c["seed"], launches=c["launches"])
        fx[f"fr_{name}_objects"], fx[f"fr_{name}_materials"] = c["objects"], c["materials"]
        fx[f"fr_{name}_camera"] = np.ascontiguousarray(c["camera"], np.float32)
        fx[f"fr_{name}_params"] = np.array([c["width"], c["height"], c["spp"], c["depth"], c["seed"], c["launches"]], np.int64)
        fx[f"fr_{name}_rgb"], fx[f"fr_{name}_states"] = rgb, st
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **fx)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {len(fx)} arrays, {size / 1e6:.2f} MB")
    assert size < 1 << 20, "a committed file stays under 1 MiB"


if __name__ == "__main__":
    main()
