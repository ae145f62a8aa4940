"""numpy restatement of pt_film_temporal (include/pt.h states the rule).

Every line of the rule is one float32 array operation per operation of the contract, in its order
(numpy neither contracts nor reorders, and keeps denormals), so the device output is held bit for bit.
A rejected tap is excluded with np.where: it is never added.  The film-owned state (the history image,
the previous camera) is an explicit value here: `temporal` takes the old one and returns the new one.
A helper, not a test module.
"""
import numpy as np

from atrous_ref import AOV_DTYPE, F

# A history pixel: three 16-byte rows {acc.rgb, len}{n, mat}{p, hit flag}
HIST_DTYPE = np.dtype([("acc", "<f4", (3,)), ("len", "<f4"), ("n", "<f4", (3,)), ("mat", "<i4"),
                       ("p", "<f4", (3,)), ("hit", "<i4")])
assert HIST_DTYPE.itemsize == 48
DEFAULTS = dict(max_history=32.0, sigma_plane=0.02, normal_cos=0.9, linear=False)

# per-pixel classes
NO_HISTORY, MISS, REJECT_K, REJECT_BOUNDS, ALL_TAPS_REJECTED, KEPT_PARTIAL, KEPT_FULL = range(7)
CLASSES = ("no film history", "miss", "rejected by k", "rejected by the frame bounds", "all taps rejected",
           "kept with fewer than 4 taps", "kept with 4 taps")
# per-tap outcomes of a pixel whose projection was kept: the first test of the rule's list that failed
TAP_NONE, TAP_OUTSIDE, TAP_PREV_MISS, TAP_MAT, TAP_NORMAL, TAP_PLANE, TAP_NONFINITE, TAP_WEIGHT, TAP_KEPT = range(9)
TAP_REASONS = {TAP_OUTSIDE: "outside the frame", TAP_PREV_MISS: "previous pixel a miss", TAP_MAT: "mat",
               TAP_NORMAL: "normal", TAP_PLANE: "plane", TAP_NONFINITE: "non-finite history"}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def temporal(rgb, aov, camera, state, W, H, max_history=32.0, sigma_plane=0.02, normal_cos=0.9, linear=False,
             debug=False):
    """One pt_film_temporal call.  rgb (n_pixels, 3) float32, aov (n_pixels,) records, camera the pt_camera
    as float32 words; state: None (no history: a new film, or after a reset) or what an earlier call
    returned.  Returns (out (n_pixels, 3), len (n_pixels,), new state, class per pixel (n_pixels,)); with
    debug=True a fifth value, a dict with `taps` (n_pixels, 4) outcomes in the rule's tap order."""
    c = np.ascontiguousarray(rgb, F).reshape(H, W, 3)
    P = np.ascontiguousarray(aov, AOV_DTYPE).reshape(H, W)
    has = state is not None and state["size"] == (W, H)
    hit_p = P["obj"] >= 0
    taps = np.full((H, W, 4), TAP_NONE, np.int8)
    with np.errstate(all="ignore"):
        cur = c if linear else c * c
        ah = np.zeros((H, W, 3), F)
        al = np.zeros((H, W), F)
        ws = np.zeros((H, W), F)
        nkept = np.zeros((H, W), np.int32)
        k_ok = np.zeros((H, W), bool)
        proj = np.zeros((H, W), bool)
        if has:
            cam = np.asarray(state["camera"], F)
            o, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
            hist = state["hist"]
            a = ll - o
            w = P["p"] - o
            cvw = _cross(ver, w)
            cwh = _cross(w, hor)
            chv = _cross(hor, ver)
            den = _dot(hor, cvw)
            u = (-_dot(a, cvw)) / den
            v = (-_dot(a, cwh)) / den
            k = _dot(a, chv) / den
            fx = u * F(W) - F(0.5)
            fy = v * F(H) - F(0.5)
            assert fx.dtype == F and k.dtype == F
            k_ok = k > 0
            proj = k_ok & (fx > -1) & (fx < F(W)) & (fy > -1) & (fy < F(H))
            base = proj & hit_p
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ix = np.where(base, x0, F(0)).astype(np.int64)
            iy = np.where(base, y0, F(0)).astype(np.int64)
            plane_lim = F(sigma_plane) * P["depth"]
            for j in range(2):
                for i in range(2):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    Q = hist[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    wq = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                    assert wq.dtype == F
                    tests = [(TAP_OUTSIDE, inside),
                             (TAP_PREV_MISS, Q["hit"] != 0),
                             (TAP_MAT, Q["mat"] == P["mat"]),
                             (TAP_NORMAL, _dot(P["n"], Q["n"]) >= F(normal_cos)),
                             (TAP_PLANE, np.abs(_dot(P["n"], Q["p"] - P["p"])) <= plane_lim),
                             (TAP_NONFINITE, (np.abs(Q["acc"][..., 0]) + np.abs(Q["acc"][..., 1])) + np.abs(Q["acc"][..., 2]) < F(np.inf)),
                             (TAP_WEIGHT, wq > 0)]
                    keep = base.copy()
                    reason = np.where(base, TAP_KEPT, TAP_NONE).astype(np.int8)
                    for code, ok in reversed(tests):   # (reversed: the first failing test of the list wins)
                        reason = np.where(base & ~ok, code, reason)
                        keep &= ok
                    taps[..., 2 * j + i] = reason
                    ah = np.where(keep[..., None], ah + wq[..., None] * Q["acc"], ah)
                    al = np.where(keep, al + wq * Q["len"], al)
                    ws = np.where(keep, ws + wq, ws)
                    nkept += keep
        have = ws > 0
        h = ah / ws[..., None]
        nh = al / ws
        length = np.where(have, np.fmin(nh + F(1), F(max_history)), F(1))
        alpha = F(1) / length
        acc = np.where(have[..., None], h + (cur - h) * alpha[..., None], cur)
        out = acc if linear else np.sqrt(acc)
    assert out.dtype == F and length.dtype == F and acc.dtype == F
    new = np.zeros((H, W), HIST_DTYPE)
    new["acc"], new["len"], new["n"], new["mat"], new["p"], new["hit"] = acc, length, P["n"], P["mat"], P["p"], hit_p
    cls = np.full((H, W), KEPT_FULL, np.int8)
    cls[nkept < 4] = KEPT_PARTIAL
    cls[nkept == 0] = ALL_TAPS_REJECTED
    cls[~proj] = REJECT_BOUNDS
    cls[~k_ok] = REJECT_K
    cls[~hit_p] = MISS
    if not has:
        cls[:] = NO_HISTORY
    assert ((nkept > 0) == have).all()
    new_state = dict(hist=new, camera=np.array(camera, F)[:12].copy(), size=(W, H))
    res = (out.reshape(-1, 3), length.reshape(-1), new_state, cls.reshape(-1))
    return res + (dict(taps=taps.reshape(-1, 4)),) if debug else res


def sequence(frames, W, H, state=None, **opts):
    """Calls in a row on one film: frames = [(rgb, aov, camera), ...] -> [(out, len, state, cls, debug), ...]."""
    res = []
    for rgb, aov, cam in frames:
        r = temporal(rgb, aov, cam, state, W, H, debug=True, **opts)
        state = r[2]
        res.append(r)
    return res


# ------------------------------------------------------------------------------------ shared test inputs
# Three nearby views of atrous_ref.lit_soup() from inside it (its triangles reach +-10), so that they cover
# a few pixels each and most hits find themselves again.
SOUP_VIEWS = ((0, 0, 9), (0.3, 0.1, 8.8), (0.6, -0.2, 8.6))
# Narrow views around synthetic_guides' slab (x, y in [-2, 2], |z| <= 0.1): many of its points project
# outside the frame, and the second camera stands inside the slab with half the points behind it.
ADVERSARIAL_VIEWS = (((0.2, -0.1, 5.0), (0.1, 0.0, 0.0), 30), ((0.0, 0.1, 0.01), (2.0, 0.4, 0.0), 60),
                     ((-3.5, 0.3, 1.0), (0.5, 0.0, 0.0), 35))


def soup_cameras(pt, W, H):
    return [pt.camera_make(frm, (0, 0, 0), 50, W / H) for frm in SOUP_VIEWS]


def adversarial_cameras(pt, W, H):
    return [pt.camera_make(frm, at, fov, W / H) for frm, at, fov in ADVERSARIAL_VIEWS]


def poison(rgb, aov):
    """A NaN channel, an inf pixel and a -inf channel on three hits of a frame (the next call then meets
    non-finite history where everything else matches)."""
    hits = np.flatnonzero(aov["obj"] >= 0)
    if len(hits) >= 3:
        rgb[hits[len(hits) // 2], 1] = np.nan
        rgb[hits[len(hits) // 3]] = np.inf
        rgb[hits[-1], 2] = -np.inf
    return rgb


def coherent_frames(pt, orc, W, H):
    """[(rgb, aov, camera words)] x 3: aov_ref records of lit_soup() from the soup cameras with random
    colours, the first frame poisoned."""
    from atrous_ref import aov_ref, lit_soup, synthetic_image
    objs, mats = lit_soup()
    frames = []
    for i, cam in enumerate(soup_cameras(pt, W, H)):
        cam = pt.camera_to_array(cam)
        aov = aov_ref(orc, objs, mats, cam, W, H)
        rgb = synthetic_image(W, H, 20 + i, special=False)
        frames.append((poison(rgb, aov) if i == 0 else rgb, aov, cam))
    return frames


def adversarial_frames(pt, W, H, seed):
    """[(rgb, aov, camera words)] x 3: synthetic_guides and synthetic_image (NaN and inf pixels where the
    frame has room for them) of three seeds under the adversarial cameras."""
    from atrous_ref import synthetic_guides, synthetic_image
    cams = [pt.camera_to_array(c) for c in adversarial_cameras(pt, W, H)]
    special = W * H > 2 * W + 2
    return [(synthetic_image(W, H, seed + i, special), synthetic_guides(W, H, seed + i), cams[i]) for i in range(3)]
