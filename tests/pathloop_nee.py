"""The render loop of tests/pathloop.py with next-event estimation (PT_RENDER_NEE) as a parameter
(a helper module, not a test file).

include/pt.h states the rule next to PT_EMISSIVE; this is its restatement, built like pathloop.py
from orc.trace, orc.scatter_tape and the stream functions.  Every value is float32 and every
operation one rounded float32 operation in the contract's order:

  lights   the objects of type 3 (triangle) whose material has type 8, in object order:
           v0, e1 = v1 - v0, e2 = v2 - v0, E.  nL == 0: the flag changes nothing (no clamp either).
  where    after the scatter of a Lambertian hit, when the path has bounces left.
  draws    uL, ua, ub -- three more uniforms of the path's stream, whatever follows.
  sample   k = min(int(uL * nL), nL - 1); fold (ua, ub) when ua + ub > 1, then ub = min(ub, 1 - ua),
           ua = min(ua, 1 - ub) (exactly inside, whatever the fold's rounded sum said); q = (v0 + ua e1) + ub e2;
           w = q - p; cs = dot(n, w); cl = |dot(cross(e1, e2), w)|; d2 = dot(w, w);
           cs <= 0, cl == 0 or d2 == 0: no ray.  Else the shadow ray (p, w) is occluded exactly when
           orc.trace(tmin = 0.001, tmax = 0.999) reports a hit; unoccluded it adds, per channel,
           ((att * albedo) * E) * G with G = ((cs * cl) * nL) / (2 pi * (d2 * d2)), NaN -> 0.
  emitters a ray scattered at a Lambertian hit that lands on an emissive TRIANGLE contributes 0.
  clamp    a finished sample is fmin(direct + ending term, 1024) per channel.

tests/test_nee_host.py proves that with nee=False (and with nee=True on a scene without emissive
triangles) this is pathloop.render / render_sample bit for bit, checks the estimator against a
quadrature, and that the NEE test scenes' paths show every case the rule has.
"""
import functools

import numpy as np

import oracle as orc
import pathloop
from pathloop import ABSORBED, DEPTH, EMITTER, F, PT_EMISSIVE, SEED, SKY, _Ctx, _block_fixed, _scatter, _sky, _uniform

PT_LAMBERTIAN, PT_TRIANGLE = 1, 3
MAX_RADIANCE = F(1024.0)
TWO_PI = F(6.2831855)
SHADOW_TMIN, SHADOW_TMAX = 0.001, 0.999

# what the rule did on a path (counted per render in result["events"])
EVENTS = ("direct_unoccluded", "direct_occluded", "direct_backfacing", "emitter_suppressed",
          "emitter_after_specular", "clamped")


def light_list(objects, materials):
    """The sampled lights: (v0, e1, e2, E), float32 (nL, 3) each, in object order."""
    objects = np.ascontiguousarray(objects, orc.OBJECT_DTYPE)
    materials = np.ascontiguousarray(materials, orc.MATERIAL_DTYPE)
    is_light = (objects["type"] == PT_TRIANGLE) & (materials["type"][objects["mat"]] == PT_EMISSIVE)
    o = objects[is_light]
    v = o["v"].astype(F).reshape(-1, 9)
    v0, v1, v2 = v[:, 0:3], v[:, 3:6], v[:, 6:9]
    return v0.copy(), (v1 - v0).astype(F), (v2 - v0).astype(F), materials["albedo"][o["mat"]].astype(F).reshape(-1, 3)


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def cross(u, v):
    return np.array([F(F(u[1] * v[2]) - F(u[2] * v[1])), F(F(u[2] * v[0]) - F(u[0] * v[2])),
                     F(F(u[0] * v[1]) - F(u[1] * v[0]))], F)


def pick_light(uL, nL):
    return min(int(F(F(uL) * F(nL))), nL - 1)


def fold(ua, ub):
    ua, ub = F(ua), F(ub)
    if F(ua + ub) > F(1.0):
        ua, ub = F(F(1.0) - ua), F(F(1.0) - ub)
    ub = min(ub, F(F(1.0) - ua))   # (a sum that rounding left an ulp beyond 1: back onto the edge)
    ua = min(ua, F(F(1.0) - ub))
    return ua, ub


def light_point(lights, k, ua, ub):
    v0, e1, e2, _ = lights
    return ((v0[k] + ua * e1[k]).astype(F) + ub * e2[k]).astype(F)


def light_sample(lights, p, n, att, uL, ua, ub):
    """(trace?, w, term): the contract's arithmetic for the uniforms (uL, ua, ub) at the hit (p, n);
    att = the attenuation after the hit (before it, times the albedo)."""
    v0, e1, e2, E = lights
    nL = len(v0)
    k = pick_light(uL, nL)
    ua, ub = fold(ua, ub)
    w = (light_point(lights, k, ua, ub) - p).astype(F)
    cs = dot(n, w)
    cl = F(abs(dot(cross(e1[k], e2[k]), w)))
    d2 = dot(w, w)
    if cs <= 0 or cl == 0 or d2 == 0:
        return False, w, np.zeros(3, F)
    with np.errstate(all="ignore"):
        G = F(F(F(cs * cl) * F(nL)) / F(TWO_PI * F(d2 * d2)))
        t = ((att * E[k]).astype(F) * G).astype(F)
    return True, w, np.where(t != t, F(0.0), t).astype(F)


def _end(total_direct, contrib, nee_on, events):
    if not nee_on:
        return contrib
    with np.errstate(all="ignore"):
        t = (total_direct + contrib).astype(F)
    if (t > MAX_RADIANCE).any():
        events["clamped"] += 1
    return np.fmin(t, MAX_RADIANCE).astype(F)


def _path(ctx, col, row, state, lights, events, shadow):
    """pathloop._path with the rule: `lights` is None (off) or a non-empty light list."""
    nee_on = lights is not None
    u = F(F(col) + F(_uniform(state.ctypes.data))) * ctx.invW
    v = F(F(row) + F(_uniform(state.ctypes.data))) * ctx.invH
    ray = ctx.ray
    ray[0, :3] = ctx.pos
    ray[0, 3:] = ((ctx.ll + u * ctx.hor) + v * ctx.ver) - ctx.pos
    att = np.ones(3, F)
    direct = np.zeros(3, F)
    from_nee = False        # the current ray left a Lambertian hit where the rule applied
    specular = False        # ... or a metal / dielectric one (bookkeeping for `events` only)
    rays = bounce = 0
    for _ in range(max(0, ctx.max_depth)):
        rays += 1
        hit = orc.trace(ctx.objects, ctx.nodes, ray, tmin=0.001)[0][0]
        if not hit["hit"]:
            return _end(direct, _sky(ctx, ray[0, 3:], att), nee_on, events), SKY, bounce, rays
        mat = ctx.materials[hit["mat"]]
        if mat["type"] == PT_EMISSIVE:   # no draw; from either side
            c = att * mat["albedo"]
            if nee_on and ctx.objects[hit["obj"]]["type"] == PT_TRIANGLE:
                if from_nee:
                    c = np.zeros(3, F)
                    events["emitter_suppressed"] += 1
                elif specular:
                    events["emitter_after_specular"] += 1
            return _end(direct, c, nee_on, events), EMITTER, bounce, rays
        n_in = hit["n"].astype(F)
        ok, out, na = _scatter(ctx, mat, ray[0], hit, state)
        if not ok:
            return _end(direct, np.zeros(3, F), nee_on, events), ABSORBED, bounce, rays
        att = att * na
        ray[0] = out
        bounce += 1
        if nee_on and bounce < ctx.max_depth:   # the path goes on: bounces left after this scatter
            from_nee = mat["type"] == PT_LAMBERTIAN
            specular = not from_nee
            if from_nee:
                uL, ua, ub = (F(_uniform(state.ctypes.data)) for _ in range(3))
                go, w, term = light_sample(lights, out[:3].astype(F), n_in, att, uL, ua, ub)
                if not go:
                    events["direct_backfacing"] += 1
                else:
                    rays += 1
                    sray = np.concatenate([out[:3], w]).astype(F).reshape(1, 6)
                    occ = bool(orc.trace(ctx.objects, ctx.nodes, sray, tmin=SHADOW_TMIN, tmax=SHADOW_TMAX)[0][0]["hit"])
                    shadow.append((sray[0].copy(), occ))
                    if occ:
                        events["direct_occluded"] += 1
                    else:
                        events["direct_unoccluded"] += 1
                        direct = (direct + term).astype(F)
    return (_end(direct, _sky(ctx, ray[0, 3:], att), nee_on, events), (DEPTH if ctx.max_depth > 0 else SKY), bounce,
            rays)


def _lights_for(objects, materials, nee):
    if not nee:
        return None
    lights = light_list(objects, materials)
    return lights if len(lights[0]) > 0 else None   # nL == 0: the flag changes nothing


def render(objects, materials, nodes, camera, width, height, rows, spp, max_depth, states, sky=pathloop.DEFAULT_SKY,
           nee=False):
    """pathloop.render with the rule as a parameter; the result has two more entries: events (how
    often each of EVENTS happened) and shadow (the traced shadow rays as (ray float32[6], occluded))."""
    ctx = _Ctx(objects, materials, nodes, camera, width, height, max_depth, sky)
    lights = _lights_for(ctx.objects, ctx.materials, nee)
    rows = np.asarray(rows, np.int64)
    states = np.ascontiguousarray(states, np.uint32).copy()
    assert states.shape == (len(rows) * width, 6)
    sums = np.zeros((len(rows) * width, 3), F)
    rays, kinds, events, shadow = 0, [], dict.fromkeys(EVENTS, 0), []
    for ri, row in enumerate(rows):
        for col in range(width):
            k = ri * width + col
            s = np.zeros(3, F)
            for _ in range(spp):
                c, kind, bounce, n = _path(ctx, col, int(row), states[k], lights, events, shadow)
                s = s + c
                rays += n
                kinds.append((kind, bounce))
            sums[k] = s
    image = np.sqrt(sums * (F(1.0) / F(spp)))
    return {"image": image, "sums": sums, "states": states, "rays": rays, "paths": len(rows) * width * spp,
            "kinds": kinds, "events": events, "shadow": shadow}


def render_sample(objects, materials, nodes, camera, width, height, rows, spp, max_depth, seed, chunk, sample_base=0,
                  sky=pathloop.DEFAULT_SKY, nee=False):
    """pathloop.render_sample with the rule as a parameter (events and shadow as in render)."""
    ctx = _Ctx(objects, materials, nodes, camera, width, height, max_depth, sky)
    lights = _lights_for(ctx.objects, ctx.materials, nee)
    rows = np.asarray(rows, np.int64)
    chunk = max(1, chunk)
    sums = np.zeros((len(rows) * width, 3), F)
    rays, kinds, events, shadow = 0, [], dict.fromkeys(EVENTS, 0), []
    for ri, row in enumerate(rows):
        for col in range(width):
            pixel = int(row) * width + col
            acc = [0, 0, 0]
            for c0 in range(0, spp, chunk):
                part = np.zeros(3, F)
                for s in range(c0, min(spp, c0 + chunk)):
                    st = orc.sample_stream(seed, sample_base + s, pixel)
                    c, kind, bounce, n = _path(ctx, col, int(row), st, lights, events, shadow)
                    part = part + c
                    rays += n
                    kinds.append((kind, bounce))
                for a in range(3):
                    acc[a] += _block_fixed(part[a])
            sums[ri * width + col] = [F(float(a) * 2.0 ** -32) for a in acc]   # fixedToFloat
    image = np.sqrt(sums * (F(1.0) / F(spp)))
    return {"image": image, "sums": sums, "rays": rays, "paths": len(rows) * width * spp, "kinds": kinds,
            "events": events, "shadow": shadow}


# ---------------------------------------------------------------- the NEE test scenes
# N1 = pathloop's L1 (cornell_lit, 24 x 24, 4 spp, depth 8, black sky): a Lambertian box under a lamp of
#      two emissive triangles.  Its paths show direct_unoccluded, direct_occluded (the two boxes' shadows),
#      direct_backfacing (the ceiling beside the lamp, faces turned away from it) and emitter_suppressed;
#      it has no metal or glass, so never emitter_after_specular.
# N2 = a variant of pathloop's L2: the same kind of soup -- random_soup(40, 12, seed, n_mat=5): triangles
#      and spheres; Lambertian, metal and dielectric; the fifth material emissive, E = (4, 3, 0.5) -- under
#      L2's sky, 24 x 16, 3 spp, depth 12, but denser (spread 3 instead of 10) and seen from outside.  L2
#      itself will not do: seen from inside its glass sphere, 953 of its 1,152 paths leave for the sky after
#      one refraction, and not one reaches a Lambertian surface with bounces left (no light sample at all).
#      Seeds 2000-2011 at spread 3 and 4 were tried on the CPU with the loop below (camera fixed at
#      (0, 1, 2.5 * spread), looking at the origin, vfov 60); seed 2007 at spread 3 was chosen because it is
#      the one whose paths show all five events at least six times each (unoccluded 34, occluded 40,
#      backfacing 56, suppressed 7, after-specular 6) and end in all five of pathloop's ways.  It has 9
#      sampled lights and 3 emissive spheres, which are not sampled and go on emitting when hit.
# Neither shows `clamped` (test_nee_host.py asserts it: the statistical GPU tests rely on that);
# clamp_scene() below is for that.
N2_SEED, N2_SPREAD = 2007, 3.0
N2_CAMERA_FROM, N2_CAMERA_AT, N2_CAMERA_VFOV = (0.0, 1.0, 7.5), (0.0, 0.0, 0.0), 60.0


@functools.lru_cache(maxsize=None)
def nee_scene(name):
    if name == "N1":
        return pathloop.lit_scene("L1")
    assert name == "N2"
    from helpers import random_soup
    objs, mats = random_soup(40, 12, N2_SEED, spread=N2_SPREAD, n_mat=5)
    mats[4]["type"] = PT_EMISSIVE
    mats[4]["albedo"] = (4.0, 3.0, 0.5)
    mats[4]["fuzz"] = mats[4]["ir"] = 0.0
    cam = orc.camera_make(N2_CAMERA_FROM, N2_CAMERA_AT, N2_CAMERA_VFOV, 24.0 / 16.0)
    return pathloop.LitScene(name, objs, mats, cam, 24, 16, 3, 12, ((0.2, 0.1, 0.3), (0.9, 0.8, 0.1)))


@functools.lru_cache(maxsize=None)
def nee_reference(name, spp=None, max_depth=None, rows=None, frames=1, seed=SEED, nee=True):
    """Compat-mode reference of an NEE scene (a list of `frames` results, each continuing the
    streams of the one before); computed once per set of arguments, shared, read-only."""
    sc = nee_scene(name)
    rows = tuple(range(sc.height)) if rows is None else rows
    states = orc.film_states(seed, sc.width, rows)
    out = []
    for _ in range(frames):
        r = render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, rows,
                   sc.spp if spp is None else spp, sc.max_depth if max_depth is None else max_depth, states,
                   sky=sc.sky, nee=nee)
        states = r["states"]
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def nee_reference_sample(name, spp=5, chunk=2, seed=SEED, nee=True):
    sc = nee_scene(name)
    return render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), spp,
                         sc.max_depth, seed, chunk, sky=sc.sky, nee=nee)


@functools.lru_cache(maxsize=None)
def clamp_scene():
    """A Lambertian floor (two triangles, albedo 0.8) with one large emissive triangle, E = (900, 900,
    900), a hair (0.05) above it under a black sky; the camera sits in the gap, just outside the lamp's
    edge, and looks along the floor, so the lower half of its 8 x 8 frame (8 spp, depth 3) sees floor
    points under the lamp.  Such a point is 0.05 from the lamp: G reaches 2 A / (2 pi 0.05^2) ~ 700
    for the lamp's area A = 5.8, times 0.8 * 900 -- far beyond PT_MAX_RADIANCE, and the sample clamps."""
    objs = np.zeros(3, orc.OBJECT_DTYPE)
    mats = np.zeros(2, orc.MATERIAL_DTYPE)
    mats[0]["type"], mats[0]["albedo"] = PT_LAMBERTIAN, (0.8, 0.8, 0.8)
    mats[1]["type"], mats[1]["albedo"] = PT_EMISSIVE, (900.0, 900.0, 900.0)
    objs["type"] = PT_TRIANGLE
    objs["mat"] = (0, 0, 1)
    objs["v"][0] = (-3, 0, -3, -3, 0, 3, 3, 0, 3)     # the floor
    objs["v"][1] = (-3, 0, -3, 3, 0, 3, 3, 0, -3)
    h = 0.05
    objs["v"][2] = (-2, h, -0.9, 2, h, -0.9, 0, h, 2)   # the lamp: its edge at z = -0.9
    cam = orc.camera_make((0.0, 0.02, -1.0), (0.0, 0.02, 0.0), 40.0, 1.0)
    return pathloop.LitScene("clamp", objs, mats, cam, 8, 8, 8, 3, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
