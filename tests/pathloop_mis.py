"""The render loop of tests/pathloop_nee.py with the light sample's and the scatter ray's weights
(PT_RENDER_MIS) as a parameter (a helper module, not a test file).

include/pt.h states the rule next to PT_RENDER_NEE; this is its restatement.  Everything of the NEE
rule stays -- the light list, where it applies, the draws, k, the fold, q, w, cs, cl, d2, the three
rejections, the shadow ray, the counters, the final clamp -- and every value is float32, every
operation one rounded float32 operation in the contract's order (pi = 3.1415927f):

  light sample  unoccluded: len = sqrt(d2); pl = ((2 * d2) * len) / (nL * cl); pb = cs / (pi * len);
                wl = pb / (pl + pb); direct += ((att * albedo) * E) * wl, NaN -> 0.
  scatter ray   at the same hit, whatever the rejections say: pbs = max(dot(n, d), 0) / (pi * sqrt(dot(d, d))),
                d = the scatter ray's unnormalised direction.
  emitters      a ray scattered at such a hit that lands on an emissive TRIANGLE at parameter t:
                wv = t * d; D2 = dot(wv, wv); L = sqrt(D2); clh = |dot(cross(e1, e2), wv)| (that
                triangle's light record); pls = ((2 * D2) * L) / (nL * clh); wb = pbs / (pls + pbs);
                the path ends with (att * E) * wb, NaN -> 0.

mis=False is pathloop_nee.render / render_sample bit for bit (tests/test_mis_host.py proves it).  The
results have pathloop_nee's keys and one more, "weights": one entry per light sample that added a term,
("light", wl, term, bound), and per weighted emitter hit, ("emitter", wb, term, bound), bound = the
term at weight 1 -- what tests/test_mis_host.py checks the rule's bounds on.
"""
import functools

import numpy as np

import oracle as orc
import pathloop
import pathloop_nee as pn
from pathloop import ABSORBED, DEPTH, EMITTER, F, PT_EMISSIVE, SEED, SKY, _Ctx, _block_fixed, _scatter, _sky, _uniform
from pathloop_nee import (EVENTS, PT_LAMBERTIAN, PT_TRIANGLE, SHADOW_TMAX, SHADOW_TMIN, clamp_scene, cross, dot, fold,
                          light_list, light_point, nee_scene, pick_light)

PI = F(3.1415927)


def light_slots(objects, materials):
    """Object index -> slot in light_list's order (meaningful for the sampled lights only)."""
    objects = np.ascontiguousarray(objects, orc.OBJECT_DTYPE)
    materials = np.ascontiguousarray(materials, orc.MATERIAL_DTYPE)
    is_light = (objects["type"] == PT_TRIANGLE) & (materials["type"][objects["mat"]] == PT_EMISSIVE)
    return np.cumsum(is_light) - is_light   # (the exclusive scan)


def light_pdf(nL, d2, cl):
    """The light sample's pdf per solid angle of a direction whose unnormalised vector w to the light's
    plane has d2 = dot(w, w) and cl = |dot(cross(e1, e2), w)|."""
    with np.errstate(all="ignore"):
        return F(F(F(F(2.0) * d2) * F(np.sqrt(d2))) / F(F(nL) * cl))


def scatter_pdf(n, d):
    """The Lambertian scatter's pdf per solid angle of the unnormalised direction d."""
    with np.errstate(all="ignore"):
        return F(max(dot(n, d), F(0.0)) / F(PI * F(np.sqrt(dot(d, d)))))


def light_sample(lights, p, n, att, uL, ua, ub, mis):
    """(trace?, w, term, weight, bound): pathloop_nee.light_sample with the weight as a parameter;
    bound = (att * E) per channel, weight = G (mis off) or wl."""
    v0, e1, e2, E = lights
    nL = len(v0)
    k = pick_light(uL, nL)
    ua, ub = fold(ua, ub)
    w = (light_point(lights, k, ua, ub) - p).astype(F)
    cs = dot(n, w)
    cl = F(abs(dot(cross(e1[k], e2[k]), w)))
    d2 = dot(w, w)
    if cs <= 0 or cl == 0 or d2 == 0:
        return False, w, np.zeros(3, F), F(0.0), np.zeros(3, F)
    with np.errstate(all="ignore"):
        if mis:
            ln = F(np.sqrt(d2))
            pl = F(F(F(F(2.0) * d2) * ln) / F(F(nL) * cl))
            pb = F(cs / F(PI * ln))
            wt = F(pb / F(pl + pb))
        else:
            wt = F(F(F(cs * cl) * F(nL)) / F(pn.TWO_PI * F(d2 * d2)))
        bound = (att * E[k]).astype(F)
        t = (bound * wt).astype(F)
    return True, w, np.where(t != t, F(0.0), t).astype(F), wt, bound


def emitter_weight(lights, slot, t, d, pbs):
    """wb of a scatter ray (direction d, pdf pbs) that hit the sampled light `slot` at parameter t."""
    _, e1, e2, _ = lights
    with np.errstate(all="ignore"):
        wv = (F(t) * d.astype(F)).astype(F)
        D2 = dot(wv, wv)
        clh = F(abs(dot(cross(e1[slot], e2[slot]), wv)))
        pls = light_pdf(len(e1), D2, clh)
        return F(pbs / F(pls + pbs))


def _path(ctx, col, row, state, lights, slots, mis, events, shadow, weights):
    """pathloop_nee._path with the weights: `lights` is None (off) or a non-empty light list."""
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
    pbs = F(0.0)            # the current ray's scatter pdf (from_nee)
    rays = bounce = 0
    for _ in range(max(0, ctx.max_depth)):
        rays += 1
        hit = orc.trace(ctx.objects, ctx.nodes, ray, tmin=0.001)[0][0]
        if not hit["hit"]:
            return pn._end(direct, _sky(ctx, ray[0, 3:], att), nee_on, events), SKY, bounce, rays
        mat = ctx.materials[hit["mat"]]
        if mat["type"] == PT_EMISSIVE:   # no draw; from either side
            c = att * mat["albedo"]
            if nee_on and ctx.objects[hit["obj"]]["type"] == PT_TRIANGLE:
                if from_nee:
                    events["emitter_suppressed"] += 1
                    if mis:
                        wb = emitter_weight(lights, int(slots[hit["obj"]]), hit["t"], ray[0, 3:], pbs)
                        with np.errstate(all="ignore"):
                            t = (c * wb).astype(F)
                        weights.append(("emitter", wb, np.where(t != t, F(0.0), t).astype(F), c.astype(F)))
                        c = weights[-1][2]
                    else:
                        c = np.zeros(3, F)
                elif specular:
                    events["emitter_after_specular"] += 1
            return pn._end(direct, c, nee_on, events), EMITTER, bounce, rays
        n_in = hit["n"].astype(F)
        ok, out, na = _scatter(ctx, mat, ray[0], hit, state)
        if not ok:
            return pn._end(direct, np.zeros(3, F), nee_on, events), ABSORBED, bounce, rays
        att = att * na
        ray[0] = out
        bounce += 1
        if nee_on and bounce < ctx.max_depth:   # the path goes on: bounces left after this scatter
            from_nee = mat["type"] == PT_LAMBERTIAN
            specular = not from_nee
            if from_nee:
                uL, ua, ub = (F(_uniform(state.ctypes.data)) for _ in range(3))
                if mis:
                    pbs = scatter_pdf(n_in, out[3:].astype(F))
                go, w, term, wt, bound = light_sample(lights, out[:3].astype(F), n_in, att, uL, ua, ub, mis)
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
                        weights.append(("light", wt, term, bound))
    return (pn._end(direct, _sky(ctx, ray[0, 3:], att), nee_on, events), (DEPTH if ctx.max_depth > 0 else SKY), bounce,
            rays)


def _setup(ctx, nee, mis):
    lights = pn._lights_for(ctx.objects, ctx.materials, nee or mis)   # (the weights imply the rule)
    return lights, (light_slots(ctx.objects, ctx.materials) if lights is not None else None)


def render(objects, materials, nodes, camera, width, height, rows, spp, max_depth, states, sky=pathloop.DEFAULT_SKY,
           nee=False, mis=False):
    """pathloop_nee.render with the weights as a parameter (mis=True implies nee)."""
    ctx = _Ctx(objects, materials, nodes, camera, width, height, max_depth, sky)
    lights, slots = _setup(ctx, nee, mis)
    rows = np.asarray(rows, np.int64)
    states = np.ascontiguousarray(states, np.uint32).copy()
    assert states.shape == (len(rows) * width, 6)
    sums = np.zeros((len(rows) * width, 3), F)
    rays, kinds, events, shadow, weights = 0, [], dict.fromkeys(EVENTS, 0), [], []
    for ri, row in enumerate(rows):
        for col in range(width):
            k = ri * width + col
            s = np.zeros(3, F)
            for _ in range(spp):
                c, kind, bounce, n = _path(ctx, col, int(row), states[k], lights, slots, mis, events, shadow, weights)
                s = s + c
                rays += n
                kinds.append((kind, bounce))
            sums[k] = s
    image = np.sqrt(sums * (F(1.0) / F(spp)))
    return {"image": image, "sums": sums, "states": states, "rays": rays, "paths": len(rows) * width * spp,
            "kinds": kinds, "events": events, "shadow": shadow, "weights": weights}


def render_sample(objects, materials, nodes, camera, width, height, rows, spp, max_depth, seed, chunk, sample_base=0,
                  sky=pathloop.DEFAULT_SKY, nee=False, mis=False, samples=None):
    """pathloop_nee.render_sample with the weights as a parameter.  `samples` (optional): a list that
    receives every sample's value (float32[3]) in pixel, then sample order."""
    ctx = _Ctx(objects, materials, nodes, camera, width, height, max_depth, sky)
    lights, slots = _setup(ctx, nee, mis)
    rows = np.asarray(rows, np.int64)
    chunk = max(1, chunk)
    sums = np.zeros((len(rows) * width, 3), F)
    rays, kinds, events, shadow, weights = 0, [], dict.fromkeys(EVENTS, 0), [], []
    for ri, row in enumerate(rows):
        for col in range(width):
            pixel = int(row) * width + col
            acc = [0, 0, 0]
            for c0 in range(0, spp, chunk):
                part = np.zeros(3, F)
                for s in range(c0, min(spp, c0 + chunk)):
                    st = orc.sample_stream(seed, sample_base + s, pixel)
                    c, kind, bounce, n = _path(ctx, col, int(row), st, lights, slots, mis, events, shadow, weights)
                    if samples is not None:
                        samples.append(np.array(c, F))
                    part = part + c
                    rays += n
                    kinds.append((kind, bounce))
                for a in range(3):
                    acc[a] += _block_fixed(part[a])
            sums[ri * width + col] = [F(float(a) * 2.0 ** -32) for a in acc]   # fixedToFloat
    image = np.sqrt(sums * (F(1.0) / F(spp)))
    return {"image": image, "sums": sums, "rays": rays, "paths": len(rows) * width * spp, "kinds": kinds,
            "events": events, "shadow": shadow, "weights": weights}


# ---------------------------------------------------------------- the MIS test scenes
# N1, N2 and clamp_scene() are pathloop_nee's.  Two more:
# rim   clamp_scene()'s geometry and camera with the lit presets' lamp radiance, E = (17, 12, 4): under
#       plain NEE 27 of its 32,768 samples (seed 5, 512 spp, depth 3) clamp and the mean is 8 standard
#       errors low on red; under the weights every light term is at most 0.8 * 17 and none clamps.
# open  the same floor with the lamp 1.0 above it and a Lambertian blocker triangle halfway, depth 4,
#       seen from (0, 0.5, -2.8): nothing near the singularity -- NEE and the weights both have the blind
#       expectation there (occluded and unoccluded samples, weights well inside (0, 1)).
RIM_E = (17.0, 12.0, 4.0)


@functools.lru_cache(maxsize=None)
def rim_scene():
    sc = clamp_scene()
    mats = sc.materials.copy()
    mats[1]["albedo"] = RIM_E
    return pathloop.LitScene("rim", sc.objects.copy(), mats, sc.camera, 8, 8, 8, 3, sc.sky)


@functools.lru_cache(maxsize=None)
def open_scene():
    objs = np.zeros(4, orc.OBJECT_DTYPE)
    mats = np.zeros(2, orc.MATERIAL_DTYPE)
    mats[0]["type"], mats[0]["albedo"] = PT_LAMBERTIAN, (0.8, 0.8, 0.8)
    mats[1]["type"], mats[1]["albedo"] = PT_EMISSIVE, RIM_E
    objs["type"] = PT_TRIANGLE
    objs["mat"] = (0, 0, 1, 0)
    objs["v"][0] = (-3, 0, -3, -3, 0, 3, 3, 0, 3)     # the floor
    objs["v"][1] = (-3, 0, -3, 3, 0, 3, 3, 0, -3)
    objs["v"][2] = (-2, 1.0, -0.9, 2, 1.0, -0.9, 0, 1.0, 2)   # the lamp, 1.0 above the floor
    objs["v"][3] = (-0.8, 0.5, -0.4, 0.8, 0.5, -0.4, 0, 0.5, 0.9)   # the blocker, halfway
    cam = orc.camera_make((0.0, 0.5, -2.8), (0.0, 0.0, 0.0), 40.0, 1.0)
    return pathloop.LitScene("open", objs, mats, cam, 8, 8, 8, 4, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))


def mis_scene(name):
    if name == "clamp":
        return clamp_scene()
    if name == "rim":
        return rim_scene()
    if name == "open":
        return open_scene()
    return nee_scene(name)


@functools.lru_cache(maxsize=None)
def mis_reference(name, spp=None, max_depth=None, rows=None, frames=1, seed=SEED, nee=True, mis=True):
    """Compat-mode reference of a scene (a list of `frames` results, each continuing the streams of
    the one before); computed once per set of arguments, shared, read-only."""
    sc = mis_scene(name)
    rows = tuple(range(sc.height)) if rows is None else rows
    states = orc.film_states(seed, sc.width, rows)
    out = []
    for _ in range(frames):
        r = render(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, rows,
                   sc.spp if spp is None else spp, sc.max_depth if max_depth is None else max_depth, states,
                   sky=sc.sky, nee=nee, mis=mis)
        states = r["states"]
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def mis_reference_sample(name, spp=5, chunk=2, seed=SEED, nee=True, mis=True):
    sc = mis_scene(name)
    return render_sample(sc.objects, sc.materials, sc.nodes, sc.camera, sc.width, sc.height, range(sc.height), spp,
                         sc.max_depth, seed, chunk, sky=sc.sky, nee=nee, mis=mis)
