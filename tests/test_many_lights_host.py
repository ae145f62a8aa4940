"""Many sampled lights, host side (no GPU): the conditions the scenes of tests/many_lights.py have to
meet so that the bit-exact GPU comparisons of tests/test_gpu_many_lights.py cannot pass vacuously, the
proof that a wrong object-to-record lookup moves the reference frame's bits, and the agreement of the
flat and the instanced restatement of the light list on these scenes."""
import numpy as np
import pytest

import instanced_lights_ref as ilr
import many_lights as ml
import pathloop_mis as pm
import pathloop_nee as pn


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _light_objects():
    sc = ml.flat_scene()
    return np.flatnonzero(ml.is_light(sc.objects, sc.materials))   # light slot -> object index


# ---------------------------------------------------------------- 1. the layout
def test_identity_split_layout():
    """What the identity split promises: at least four light-bearing meshes of different sizes, a
    lightless mesh with Lambertian, metal and glass objects and spheres, an empty mesh; mesh ranges not
    ascending, instance order unlike mesh order, the lightless instance first, the empty mesh between
    light-bearing instances and last; 4,500 objects (no power of two), every non-empty mesh once.
    Lights: 905 = L 0, A 360, B 101, C 266, D 178; per scan tile of the flattened array 411, 418, 76."""
    objs, first, count, inst, mats = ml.instanced_identity_scene()
    n = len(objs)
    assert n == 4500 and n & (n - 1) != 0 and int(count.sum()) == n
    assert (np.diff(first) < 0).any() and first[0] != first[count > 0].min()   # mesh 0 is not the first range
    order = inst["mesh"].tolist()
    assert order != sorted(order) and len(order) == 8
    nonempty = [m for m in order if count[m] > 0]
    assert sorted(nonempty) == sorted(np.flatnonzero(count > 0).tolist())     # each non-empty mesh exactly once
    per_mesh = [int(ml.is_light(objs[f:f + c], mats).sum()) for f, c in zip(first, count)]
    per_inst = [per_mesh[m] for m in order]
    assert per_inst == [0, 360, 0, 101, 266, 0, 178, 0]
    assert [int(count[m]) for m in order] == [300, 1500, 0, 500, 1300, 0, 900, 0]
    dark = objs[first[order[0]]:first[order[0]] + count[order[0]]]
    assert set(mats["type"][dark["mat"][dark["type"] == 3]].tolist()) == {1, 2, 4}   # Lambertian, metal, glass triangles
    assert (dark["type"] == 1).sum() >= 3
    sc = ml.flat_scene()
    lit = ml.is_light(sc.objects, sc.materials)
    assert [int(lit[t:t + ml.SCAN_TILE].sum()) for t in range(0, n, ml.SCAN_TILE)] == [411, 418, 76]
    assert lit.sum() == 905
    assert ((sc.objects["type"] == 1) & (sc.materials["type"][sc.objects["mat"]] == 8)).sum() > 0   # emissive spheres


def test_transformed_scene_layout():
    """536 records = 2 * 256 + 24: three blocks of the record kernel.  First records per instance 0, 0, 0, 106,
    109, 109, 215, 215, 321, 324, 430, 536, 536: lightless and empty-mesh instances first, between and
    last, and no light-bearing instance after the first starts on a multiple of 256.  The big mesh's 106
    emissive triangles are interleaved with its other objects and carry two radiances.  nL does not
    depend on the matrices."""
    objs, first, count, inst, mats = ml.instanced_transformed_scene()
    per_mesh = [int(ml.is_light(objs[f:f + c], mats).sum()) for f, c in zip(first, count)]
    assert per_mesh == [106, 0, 0, 3] and count.tolist() == [316, 0, 46, 5] and first[0] != 0
    per_inst = np.array([per_mesh[m] for m in inst["mesh"]])
    starts = np.concatenate([[0], np.cumsum(per_inst)])
    assert starts.tolist() == [0, 0, 0, 106, 109, 109, 215, 215, 321, 324, 430, 536, 536, 536]
    nL = int(starts[-1])
    assert nL > 2 * ml.BLOCK and (nL + ml.BLOCK - 1) // ml.BLOCK == 3
    assert all(s % ml.BLOCK != 0 for s, c in zip(starts[:-1], per_inst) if c > 0 and s > 0)
    assert per_inst[0] == 0 and per_inst[-1] == 0 and (per_inst[1:-1] == 0).sum() >= 3
    big = objs[first[0]:first[0] + count[0]]
    lit = ml.is_light(big, mats)
    runs = np.flatnonzero(np.diff(lit.astype(int)) != 0)
    assert len(runs) > 100                                       # interleaved, not one run
    assert set(big["mat"][lit].tolist()) == {4, 5} and (mats["albedo"][4] != mats["albedo"][5]).all()
    lights = ilr.light_list(objs, first, count, inst, mats)
    assert len(lights[0]) == nL
    for other in (ml.moved(inst), ):
        got = ilr.light_list(objs, first, count, other, mats)
        assert len(got[0]) == nL
        changed = np.flatnonzero((bits(got[0]) != bits(lights[0])).any(1))
        a, b = ml.XF_MOVED
        assert changed.min() == starts[a] and changed.max() == starts[b] - 1 and len(changed) == starts[b] - starts[a]
    ident = inst.copy()
    ident["m"][:] = ilr.IDENT
    assert len(ilr.light_list(objs, first, count, ident, mats)[0]) == nL
    # the matrices hold a mirror (det < 0) and two that are no similarity (the stretch and the shear)
    lin = inst["m"].reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    assert (np.linalg.det(lin) < 0).sum() == 1
    sv = np.linalg.svd(lin, compute_uv=False)
    assert ((sv[:, 0] / sv[:, 2]) > 1.2).sum() >= 2
    one = ml.instanced_transformed_scene(single=True)
    assert len(one[3]) == 1 and len(ilr.light_list(*one)[0]) == 106


# ---------------------------------------------------------------- 2. what the reference frames show
@pytest.mark.parametrize("sample", [False, True], ids=["compat", "sample"])
def test_flat_reference_shows_every_case(sample):
    """The flat soup's reference frames, 32 x 24, depth 12 (compat: 3 spp from film seed 21; sample: 5 spp,
    chunk 2): every event of the rule but `clamped` at least 20 times, `clamped` never, at least 20
    weighted emitter hits, the picked lights in the first and the last scan tile and at least 100
    distinct, and at least 3 scatter-ray hits on the lights of every light-bearing mesh of the identity
    split.  The NEE and the MIS frame draw the same numbers, so they show the same events and picks.
    Achieved, compat: unoccluded 107, occluded 293, back-facing 425, suppressed / weighted emitter hits 58,
    after specular 64; 825 picks of 540 distinct lights, from light 0 to light 903 of 905, in all three
    tiles; hits per mesh A 21, B 5, C 19, D 13; 4,252 rays.
    Sample: 182, 456, 719, 110, 106; 1,357 picks of 698 distinct lights; hits A 39, B 9, C 30, D 32; 7,080 rays.
    (Seeds 3002-3004 meet the conditions too; at spread 18 no scatter ray finds mesh B's lights.)"""
    nee, mis = ml.flat_reference(False, sample), ml.flat_reference(True, sample)
    print("events", mis["events"], "rays", mis["rays"])
    assert nee["events"] == mis["events"] and nee["picks"] == mis["picks"] and nee["rays"] == mis["rays"]
    assert nee["kinds"] == mis["kinds"] and (bits(nee["image"]) != bits(mis["image"])).any()
    for name in pn.EVENTS:
        if name == "clamped":
            assert mis["events"][name] == 0
        else:
            assert mis["events"][name] >= 20, name
    emitter = [w for w in mis["weights"] if w[0] == "emitter"]
    assert len(emitter) == nee["events"]["emitter_suppressed"] == len(mis["hits"]) >= 20
    assert not any(w[0] == "emitter" for w in nee["weights"])
    light_obj = _light_objects()
    nL = len(light_obj)
    picks = np.array(mis["picks"])
    assert len(picks) == sum(mis["events"][k] for k in ("direct_unoccluded", "direct_occluded", "direct_backfacing"))
    assert picks.min() >= 0 and picks.max() < nL and nL & (nL - 1) != 0
    tiles = set((light_obj[picks] // ml.SCAN_TILE).tolist())
    print("picks", len(picks), "distinct", len(set(picks.tolist())), "min", picks.min(), "max", picks.max(), "tiles", tiles)
    assert tiles == {0, 1, 2} and len(set(picks.tolist())) >= 100
    hit_obj = light_obj[np.array(mis["hits"], np.int64)]
    per = {p: int(((hit_obj >= a) & (hit_obj < b)).sum()) for p, (a, b) in ml.flat_part_ranges().items()}
    print("scatter-ray hits per mesh", per)
    assert per["L"] == 0 and all(per[p] >= 3 for p in ml.LIGHT_PARTS)
    if not sample:
        assert picks.min() == 0   # light 0 is drawn in the compat frame


# ---------------------------------------------------------------- 3. teeth
def _wrong_tables():
    sc = ml.flat_scene()
    slots = pm.light_slots(sc.objects, sc.materials)
    lit = ml.is_light(sc.objects, sc.materials)
    nL = int(lit.sum())
    shifted = np.where(lit, (slots + 1) % nL, slots)
    # what exchanging two instances' first records would do: B's lights looked up from D's start and
    # D's from B's (both stay inside the list: B has 101 lights, D 178, and C's 266 follow B)
    rng = ml.flat_part_ranges()
    in_b, in_d = (np.zeros(len(lit), bool) for _ in range(2))
    in_b[rng["B"][0]:rng["B"][1]] = True
    in_d[rng["D"][0]:rng["D"][1]] = True
    first_b, first_d = int(slots[rng["B"][0]]), int(slots[rng["D"][0]])
    swapped = slots.copy()
    swapped[lit & in_b] += first_d - first_b
    swapped[lit & in_d] += first_b - first_d
    assert swapped[lit].min() >= 0 and swapped[lit].max() < nL
    assert (swapped[lit & ~in_b & ~in_d] == slots[lit & ~in_b & ~in_d]).all()
    return {"shifted": shifted, "swapped": swapped}


@pytest.mark.parametrize("table", ["shifted", "swapped"])
@pytest.mark.parametrize("sample", [False, True], ids=["compat", "sample"])
def test_a_wrong_slot_table_moves_the_frames_bits(table, sample):
    """The MIS reference rendered with a wrong object-to-record table -- every light's slot + 1 modulo nL,
    or only mesh B's and mesh D's lights looked up from each other's first record -- differs from the
    right frame in its bits; rays, streams and events stay (the lookup feeds a weight only).  So the
    bit-exact GPU frames fail on a wrong slot, rank or first-record table.
    Pixels of 768 whose bits change: shifted 55 (compat) and 96 (sample); swapped 17 and 40.  The image
    mean moves by 0.12 to 0.31 %: the tolerance bars of the instanced tests could not see it."""
    right = ml.flat_reference(True, sample)
    wrong = ml.render_flat(ml.flat_scene(), True, sample, slots=_wrong_tables()[table])
    changed = int((bits(right["image"]) != bits(wrong["image"])).any(1).sum())
    mean = float(np.abs(wrong["image"].mean() / right["image"].mean() - 1.0))
    print(table, "sample" if sample else "compat", "pixels changed", changed, "of", len(right["image"]),
          "mean moves by", mean)
    assert changed > 0
    assert wrong["rays"] == right["rays"] and wrong["events"] == right["events"] and wrong["picks"] == right["picks"]
    if not sample:
        np.testing.assert_array_equal(wrong["states"], right["states"])


def test_recorder_leaves_the_loop_alone():
    """The frames of many_lights.render_flat are pathloop_mis.render's and pathloop_nee.render's own."""
    sc = ml.flat_scene()
    st = pn.orc.film_states(ml.SEED, sc.width, range(sc.height))
    for mis in (False, True):
        mine = ml.flat_reference(mis)
        if mis:
            ref = pm.render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), sc.spp,
                            sc.max_depth, st, sky=sc.sky, mis=True)
        else:
            ref = pn.render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), sc.spp,
                            sc.max_depth, st, sky=sc.sky, nee=True)
        np.testing.assert_array_equal(bits(mine["image"]), bits(ref["image"]))
        np.testing.assert_array_equal(mine["states"], ref["states"])
        assert mine["rays"] == ref["rays"] and mine["events"] == ref["events"]
    assert pm.pick_light is pn.pick_light   # (the recorders are gone)


# ---------------------------------------------------------------- 4. the restatements agree
def test_identity_split_lists_the_flat_lights():
    objs, first, count, inst, mats = ml.instanced_identity_scene()
    flat = ml.flattened(objs, first, count, inst)
    np.testing.assert_array_equal(flat, ml.flat_scene().objects)
    want = pn.light_list(flat, mats)
    got = ilr.light_list(objs, first, count, inst, mats)
    assert len(got[0]) == len(want[0]) == 905
    for g, w in zip(got, want):
        np.testing.assert_array_equal(bits(g), bits(w))
    assert sorted(map(tuple, flat["v"].tolist())) == sorted(map(tuple, objs["v"].tolist()))   # a permutation of the array


# ---------------------------------------------------------------- 5. the edge-list generator
EDGE_NS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 6145)


@pytest.mark.parametrize("n", EDGE_NS)
def test_edge_list_scene_counts(n):
    """The list restatement counts what each pattern says (written out here, not taken from the generator)."""
    spheres = 3 if n >= 16 else 0
    want = {"all": n - spheres, "none": 0, "first_only": 1, "last_only": 1,
            "alternate": (n + 1) // 2 - (1 if spheres else 0) - (1 if spheres and (n // 2 + 1) % 2 == 0 else 0)
            - (1 if spheres and (n - 3) % 2 == 0 else 0),
            "tile_ends": sum(1 for i in (2047, 2048, 4095, 4096) if i < n)}
    pats = ml.edge_patterns(n)
    assert set(pats) >= {"all", "none", "first_only", "last_only"}
    assert ("alternate" in pats) == (n >= 2) and ("tile_ends" in pats) == (n >= 2048)
    for p in pats:
        objs, mats = ml.edge_list_scene(n, p)
        assert len(objs) == n and (objs["type"] == 1).sum() == spheres
        assert (mats["type"][objs["mat"][objs["type"] == 1]] == 8).all()          # the spheres are emissive
        v0, e1, e2, E = pn.light_list(objs, mats)
        assert len(v0) == want[p], (n, p)
        lit = np.flatnonzero(ml.is_light(objs, mats))
        assert lit.tolist() == ml.edge_light_indices(n, p)
        if p == "first_only":
            assert lit.tolist() == [0]
        if p == "last_only":
            assert lit.tolist() == [n - 1]
        if p == "tile_ends":
            assert lit.tolist() == [i for i in (2047, 2048, 4095, 4096) if i < n]
        if len(v0) > 1:
            assert len({tuple(x) for x in v0.tolist()}) == len(v0)                 # distinct triangles
            assert len({tuple(x) for x in E.tolist()}) == 2                        # both radiances listed
        area = np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1)
        assert (area > 0.1).all()


# ---------------------------------------------------------------- 6. the growth walk
def test_growth_steps_counts():
    """2, 905, 0, 838 and 5 lights over one geometry; the second 'many' step lists other triangles than
    the first, and the five-light step has the first and the last light and both sides of a tile's end."""
    sc = ml.flat_scene()
    steps = ml.growth_steps()
    lit = [ml.is_light(o, sc.materials) for o in steps]
    assert [int(x.sum()) for x in lit] == [2, 905, 0, 838, 5]
    assert not (lit[1] & lit[3]).any()
    for o in steps:
        np.testing.assert_array_equal(o["v"], sc.objects["v"])
        np.testing.assert_array_equal(o["type"], sc.objects["type"])
    all_lit, five = np.flatnonzero(lit[1]), np.flatnonzero(lit[4])
    assert five[0] == all_lit[0] and five[-1] == all_lit[-1]
    assert five[1] < ml.SCAN_TILE <= five[2] and five[3] < 2 * ml.SCAN_TILE
    assert set(five.tolist()) <= set(all_lit.tolist())
