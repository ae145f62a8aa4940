"""The render loop restated in Python out of oracle parts (a helper module, not a test file).

oracle/ knows one light, the reference's sky, and absorbs every material type it does not know.
Emissive materials (PT_EMISSIVE = 8) and a per-scene sky are additions of this project, so their
exact reference cannot come from orc.render.  This module rebuilds the loop of orc_render3 /
tracePath (oracle/pt_oracle.cpp) from the parts the oracle exposes -- the XORWOW and Philox stream
functions, orc.trace for the closest hit, orc.scatter_tape for the three materials -- and adds the
two rules as parameters of the loop:

  * a hit on a material of type 8 ends the path with att * E (E = the material's albedo slot), one
    fp32 multiply per channel, and draws nothing;
  * a miss, or a path out of bounces, returns ((1 - t) * H + t * Z) * att, t = 0.5 * (ud.y + 1), in
    the oracle's operation order; H = (1, 1, 1), Z = (0.5, 0.7, 1) is the oracle's sky.

Every value is float32 and every operation is one rounded float32 operation in the oracle's order
(the oracle is built with contraction off).  tests/test_emission_host.py first proves the
restatement against orc.render / orc.render_sample bit for bit (no emitter, default sky); only
then do the lit frames it produces count as a reference.
"""
import functools

import numpy as np

import oracle as orc

F = np.float32
PT_EMISSIVE = 8
DEFAULT_SKY = ((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))

# how a path ended; `bounce` (the number of scatterings before the end) goes with each
SKY, ABSORBED, DEPTH, EMITTER = 0, 1, 2, 3

_uniform = orc.lib.orc_curand_uniform


class _Ctx:
    def __init__(self, objects, materials, nodes, camera, width, height, max_depth, sky):
        self.objects = np.ascontiguousarray(objects, orc.OBJECT_DTYPE)
        self.materials = np.ascontiguousarray(materials, orc.MATERIAL_DTYPE)
        self.nodes = nodes
        cam = np.ascontiguousarray(camera, F)
        assert cam.shape == (orc.CAMERA_FLOATS,) and cam[22] == 0, "pinhole cameras only (lens_radius == 0)"
        self.pos, self.ll, self.hor, self.ver = cam[0:3].copy(), cam[3:6].copy(), cam[6:9].copy(), cam[9:12].copy()
        self.invW, self.invH = F(1.0) / F(width), F(1.0) / F(height)   # main.cu:281
        self.max_depth = max_depth
        self.H, self.Z = np.asarray(sky[0], F), np.asarray(sky[1], F)
        assert self.H.shape == (3,) and self.Z.shape == (3,)
        self.ray = np.zeros((1, 6), F)


def _sky(ctx, d, att):
    """normalize (vec3.h:100-104: v * (1 / length)), then the blend and the attenuation."""
    length = np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    udy = F(0.0) if length == 0 else F(F(1.0) / length) * d[1]
    t = F(0.5) * F(udy + F(1.0))
    return (F(F(1.0) - t) * ctx.H + t * ctx.Z) * att


def _scatter(ctx, mat, ray, hit, state):
    """orc.scatter_tape on uniforms drawn from a copy of the stream; the stream itself then advances
    by the draws the material used."""
    n = 32
    while True:
        tape = orc.curand_uniform(state.copy(), n)
        ok, out, att, used = orc.scatter_tape(mat, ray, hit, tape)
        if used < len(tape):
            break
        n *= 2   # the tape ran out (a long rejection loop): a longer one, same stream
    for _ in range(used):
        _uniform(state.ctypes.data)
    return ok, out, att


def _path(ctx, col, row, state):
    """One camera sample of pixel (col, row) from the stream `state` (advanced in place):
    (contribution float32[3], ending kind, bounces before the end, rays traced)."""
    u = F(F(col) + F(_uniform(state.ctypes.data))) * ctx.invW
    v = F(F(row) + F(_uniform(state.ctypes.data))) * ctx.invH
    ray = ctx.ray
    ray[0, :3] = ctx.pos
    ray[0, 3:] = ((ctx.ll + u * ctx.hor) + v * ctx.ver) - ctx.pos
    att = np.ones(3, F)
    rays = bounce = 0
    for _ in range(max(0, ctx.max_depth)):
        rays += 1
        hit = orc.trace(ctx.objects, ctx.nodes, ray, tmin=0.001)[0][0]
        if not hit["hit"]:
            return _sky(ctx, ray[0, 3:], att), SKY, bounce, rays
        mat = ctx.materials[hit["mat"]]
        if mat["type"] == PT_EMISSIVE:   # no draw; from either side
            return att * mat["albedo"], EMITTER, bounce, rays
        ok, out, na = _scatter(ctx, mat, ray[0], hit, state)
        if not ok:
            return np.zeros(3, F), ABSORBED, bounce, rays
        att = att * na
        ray[0] = out
        bounce += 1
    return _sky(ctx, ray[0, 3:], att), (DEPTH if ctx.max_depth > 0 else SKY), bounce, rays


def render(objects, materials, nodes, camera, width, height, rows, spp, max_depth, states, sky=DEFAULT_SKY):
    """Compat mode, like orc.render: one XORWOW stream per pixel of `rows`, samples in order.
    `states` ((npix, 6) uint32) is left alone; the advanced streams are returned.  Returns a dict:
    image (sqrt(sum * (1 / spp))), sums (the raw per-pixel sums), states, rays, paths and kinds --
    one (kind, bounce) per path, pixels in order, samples in order."""
    ctx = _Ctx(objects, materials, nodes, camera, width, height, max_depth, sky)
    rows = np.asarray(rows, np.int64)
    states = np.ascontiguousarray(states, np.uint32).copy()
    assert states.shape == (len(rows) * width, 6)
    sums = np.zeros((len(rows) * width, 3), F)
    rays, kinds = 0, []
    for ri, row in enumerate(rows):
        for col in range(width):
            k = ri * width + col
            s = np.zeros(3, F)
            for _ in range(spp):
                c, kind, bounce, n = _path(ctx, col, int(row), states[k])
                s = s + c
                rays += n
                kinds.append((kind, bounce))
            sums[k] = s
    image = np.sqrt(sums * (F(1.0) / F(spp)))
    return {"image": image, "sums": sums, "states": states, "rays": rays, "paths": len(rows) * width * spp,
            "kinds": kinds}


def _block_fixed(x):
    """blockFixed (pt_oracle.cpp): a block's fp32 sum as a 32.32 fixed-point integer, truncated."""
    p = F(x) * F(4294967296.0)
    if p != p:
        p = F(0.0)
    p = min(max(p, F(-4611686018427387904.0)), F(4611686018427387904.0))
    return int(p)


def render_sample(objects, materials, nodes, camera, width, height, rows, spp, max_depth, seed, chunk,
                  sample_base=0, sky=DEFAULT_SKY):
    """Sample mode, like orc.render_sample / orc_render_sample2: one stream per pixel-sample, blocks
    of `chunk` samples summed in fp32, the blocks added as 32.32 fixed-point integers.  Returns a
    dict: image, sums (the resolved per-pixel totals), rays, paths, kinds."""
    ctx = _Ctx(objects, materials, nodes, camera, width, height, max_depth, sky)
    rows = np.asarray(rows, np.int64)
    chunk = max(1, chunk)
    sums = np.zeros((len(rows) * width, 3), F)
    rays, kinds = 0, []
    for ri, row in enumerate(rows):
        for col in range(width):
            pixel = int(row) * width + col
            acc = [0, 0, 0]
            for c0 in range(0, spp, chunk):
                part = np.zeros(3, F)
                for s in range(c0, min(spp, c0 + chunk)):
                    st = orc.sample_stream(seed, sample_base + s, pixel)
                    c, kind, bounce, n = _path(ctx, col, int(row), st)
                    part = part + c
                    rays += n
                    kinds.append((kind, bounce))
                for a in range(3):
                    acc[a] += _block_fixed(part[a])
            sums[ri * width + col] = [F(float(a) * 2.0 ** -32) for a in acc]   # fixedToFloat
    image = np.sqrt(sums * (F(1.0) / F(spp)))
    return {"image": image, "sums": sums, "rays": rays, "paths": len(rows) * width * spp, "kinds": kinds}


def ending_kinds(kinds):
    """The set of endings in a render's `kinds`: 'sky', 'absorbed', 'depth', 'emitter_primary',
    'emitter_bounced'."""
    out = set()
    for kind, bounce in kinds:
        if kind == EMITTER:
            out.add("emitter_primary" if bounce == 0 else "emitter_bounced")
        else:
            out.add({SKY: "sky", ABSORBED: "absorbed", DEPTH: "depth"}[kind])
    return out


ALL_ENDINGS = {"sky", "absorbed", "depth", "emitter_primary", "emitter_bounced"}


# ---------------------------------------------------------------- the two lit test scenes
class LitScene:
    """Arrays, camera, frame and sky of a lit test scene, plus its LBVH for the loop above."""

    def __init__(self, name, objects, materials, camera, width, height, spp, max_depth, sky):
        self.name, self.objects, self.materials = name, objects, materials
        self.camera = np.ascontiguousarray(camera, F)   # the oracle's 25 floats (= bytes of pt_camera)
        self.width, self.height, self.spp, self.max_depth, self.sky = width, height, spp, max_depth, sky
        self.nodes = orc.build_lbvh(objects, orc.morton_keys(objects), tight=True)


# L2's soup and camera, chosen (by a search over seeds, on the CPU, with the loop above) so that its
# 1,152 paths end in every way -- test_emission_host.py checks that.  A sparse soup seen from outside
# has next to no path that runs out of bounces or starts on an emitter, so the camera sits inside one
# of the soup's glass spheres, off-centre (total internal reflection traps part of its rays for good:
# the depth endings; the rest leave for the sky or the soup), and looks at an emissive triangle that
# reaches into that sphere (the primary emitter hits).
L2_SEED = 1941
L2_CAMERA_FROM = (-0.7606797218322754, -3.7550902366638184, 9.920369148254395)
L2_CAMERA_AT = (-0.7577590346336365, -4.791014194488525, 9.05327320098877)
L2_CAMERA_VFOV = 90.0


@functools.lru_cache(maxsize=None)
def lit_scene(name):
    """L1: the cornell_lit preset at 24 x 24, 4 spp, depth 8, under a black sky.
    L2: random_soup(40, 12, L2_SEED, n_mat=5) -- triangles and spheres, Lambertian, metal and
    dielectric -- with the fifth material emissive, E = (4, 3, 0.5), under the sky H = (0.2, 0.1, 0.3),
    Z = (0.9, 0.8, 0.1), 24 x 16, 3 spp, depth 12, seen by the camera L2_CAMERA_* above."""
    import ptamd
    from helpers import random_soup
    if name == "L1":
        p = ptamd.Preset("cornell_lit", 24, 24)
        return LitScene(name, p.objects, p.materials, ptamd.camera_to_array(p.camera), 24, 24, 4, 8,
                        (tuple(float(x) for x in p.sky[0]), tuple(float(x) for x in p.sky[1])))
    assert name == "L2"
    objs, mats = random_soup(40, 12, L2_SEED, n_mat=5)
    mats[4]["type"] = PT_EMISSIVE
    mats[4]["albedo"] = (4.0, 3.0, 0.5)
    mats[4]["fuzz"] = mats[4]["ir"] = 0.0
    cam = orc.camera_make(L2_CAMERA_FROM, L2_CAMERA_AT, L2_CAMERA_VFOV, 24.0 / 16.0)
    return LitScene(name, objs, mats, cam, 24, 16, 3, 12, ((0.2, 0.1, 0.3), (0.9, 0.8, 0.1)))


SEED = 21   # film seed of the lit tests


@functools.lru_cache(maxsize=None)
def lit_reference(name, spp=None, max_depth=None, rows=None, frames=1, sky=None, seed=SEED):
    """Compat-mode reference of a lit scene, computed once per set of arguments and shared: a list
    of `frames` render() results, each continuing the streams of the one before.  Treat as read-only."""
    sc = lit_scene(name)
    rows = tuple(range(sc.height)) if rows is None else rows
    states = orc.film_states(seed, sc.width, rows)
    out = []
    for _ in range(frames):
        r = render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, rows,
                   sc.spp if spp is None else spp, sc.max_depth if max_depth is None else max_depth, states,
                   sky=sc.sky if sky is None else sky)
        states = r["states"]
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def lit_reference_sample(name, spp=5, chunk=2, seed=SEED):
    sc = lit_scene(name)
    return render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), spp,
                         sc.max_depth, seed, chunk, sky=sc.sky)
