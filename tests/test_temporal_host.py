"""pt_film_temporal's rule on the CPU: the numpy restatement (tests/temporal_ref.py, what the GPU tests
hold the kernel to bit for bit) against a plain per-pixel loop that follows include/pt.h line by line,
the inputs' coverage of every branch of the rule, the filter's invariants, and the condition that it
helps at all: along a camera dolly the history is closer to a 1024-spp frame than the last noisy frame.
"""
import numpy as np
import pytest

import atrous_ref
import temporal_ref as tr
from atrous_ref import F

INF = F(np.inf)


# --------------------------------------------------------------------------------- the per-pixel loop
def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def loop_temporal(rgb, aov, camera, state, W, H, max_history, sigma_plane, normal_cos, linear):
    """include/pt.h's rule, pixel by pixel and tap by tap, in np.float32 scalars.  state: None or
    (history records (H, W), previous camera words)."""
    c = np.asarray(rgb, F).reshape(H, W, 3)
    g = aov.reshape(H, W)
    out = np.zeros((H, W, 3), F)
    length = np.zeros((H, W), F)
    new = np.zeros((H, W), tr.HIST_DTYPE)
    for y in range(H):
        for x in range(W):
            P = g[y, x]
            cur = [c[y, x, ch] if linear else c[y, x, ch] * c[y, x, ch] for ch in range(3)]
            ah, al, ws = [F(0), F(0), F(0)], F(0), F(0)
            if state is not None and P["obj"] >= 0:
                hist, cam = state
                o, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
                a = ll - o
                w = P["p"] - o
                cvw, cwh, chv = cross(ver, w), cross(w, hor), cross(hor, ver)
                den = dot(hor, cvw)
                u = (-dot(a, cvw)) / den
                v = (-dot(a, cwh)) / den
                k = dot(a, chv) / den
                fx = u * F(W) - F(0.5)
                fy = v * F(H) - F(0.5)
                if k > 0 and fx > -1 and fx < F(W) and fy > -1 and fy < F(H):
                    x0, y0 = np.floor(fx), np.floor(fy)
                    tx, ty = fx - x0, fy - y0
                    for j in range(2):
                        for i in range(2):
                            qx, qy = int(x0) + i, int(y0) + j
                            if qx < 0 or qx >= W or qy < 0 or qy >= H:
                                continue
                            wq = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                            Q = hist[qy, qx]
                            if not Q["hit"]:
                                continue
                            if not Q["mat"] == P["mat"]:
                                continue
                            if not dot(P["n"], Q["n"]) >= F(normal_cos):
                                continue
                            if not np.abs(dot(P["n"], Q["p"] - P["p"])) <= F(sigma_plane) * P["depth"]:
                                continue
                            if not (np.abs(Q["acc"][0]) + np.abs(Q["acc"][1])) + np.abs(Q["acc"][2]) < INF:
                                continue
                            if not wq > 0:
                                continue
                            for ch in range(3):
                                ah[ch] = ah[ch] + wq * Q["acc"][ch]
                            al = al + wq * Q["len"]
                            ws = ws + wq
            have = ws > 0
            ln = np.fmin(al / ws + F(1), F(max_history)) if have else F(1)
            alpha = F(1) / ln
            for ch in range(3):
                if have:
                    h = ah[ch] / ws
                    acc = h + (cur[ch] - h) * alpha
                else:
                    acc = cur[ch]
                new[y, x]["acc"][ch] = acc
                out[y, x, ch] = acc if linear else np.sqrt(acc)
            length[y, x] = ln
            new[y, x]["len"] = ln
            new[y, x]["n"], new[y, x]["mat"], new[y, x]["p"], new[y, x]["hit"] = P["n"], P["mat"], P["p"], P["obj"] >= 0
    assert out.dtype == F and length.dtype == F
    return out.reshape(-1, 3), length.reshape(-1), (new, np.asarray(camera, F)[:12].copy())


# -------------------------------------------------------------------------------------------- inputs
coherent_frames, adversarial_frames = tr.coherent_frames, tr.adversarial_frames


@pytest.fixture(autouse=True)
def binding_has_the_call(pt):
    """What this module restates exists in the library and its binding (with the restatement's defaults)."""
    assert hasattr(pt.lib, "pt_film_temporal") and callable(pt.temporal) and pt.TemporalOpts
    import inspect
    sig = inspect.signature(pt.temporal).parameters
    assert {k: sig[k].default for k in tr.DEFAULTS} == tr.DEFAULTS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_loop(frames, W, H, **opts):
    state, res = None, []
    for rgb, aov, cam in frames:
        out, ln, state = loop_temporal(rgb, aov, cam, state, W, H, **opts)
        res.append((out, ln, state[0]))
    return res


OPTS = dict(max_history=32.0, sigma_plane=0.02, normal_cos=0.9, linear=False)
LOOP_CASES = [("coherent", 7, 5, dict(OPTS, max_history=2.0)), ("coherent", 5, 3, OPTS),
              ("adversarial", 7, 5, dict(OPTS, max_history=2.0, normal_cos=0.5)), ("adversarial", 5, 3, dict(OPTS, sigma_plane=0.1)),
              ("adversarial", 7, 5, dict(OPTS, linear=True, sigma_plane=0.05))]


@pytest.mark.parametrize("kind,W,H,opts", LOOP_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(LOOP_CASES)])
def test_restatement_equals_loop(pt, orc, kind, W, H, opts):
    frames = coherent_frames(pt, orc, W, H) if kind == "coherent" else adversarial_frames(pt, W, H, 3)
    with np.errstate(all="ignore"):
        want = run_loop(frames, W, H, **opts)
    got = tr.sequence(frames, W, H, **opts)
    for call, ((out, ln, st, _, _), (lout, lln, lhist)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(bits(out), bits(lout), err_msg=f"call {call}")
        np.testing.assert_array_equal(bits(ln), bits(lln), err_msg=f"call {call}")
        assert st["hist"].tobytes() == lhist.tobytes(), f"call {call}"


def test_max_history_clamp_binds_on_the_third_call(pt, orc):
    """(of the loop cases' first sequence: without the clamp its third call reaches lengths above 2)"""
    W, H = 7, 5
    res = tr.sequence(coherent_frames(pt, orc, W, H), W, H, **dict(OPTS, max_history=2.0))
    assert res[1][1].max() == 2.0 and res[2][1].max() == 2.0
    free = tr.sequence(coherent_frames(pt, orc, W, H), W, H, **OPTS)
    assert free[2][1].max() > 2.0


def coverage_runs(pt, orc):
    """Every sequence the coverage condition is asserted over (sizes the GPU tests use too)."""
    runs = [tr.sequence(coherent_frames(pt, orc, W, H), W, H, **OPTS) for W, H in ((7, 5), (37, 23))]
    runs += [tr.sequence(adversarial_frames(pt, W, H, 3), W, H, **dict(OPTS, sigma_plane=0.05, normal_cos=0.5))
             for W, H in ((7, 5), (37, 23), (70, 45))]
    return runs


def test_inputs_reach_every_class_and_every_tap_reason(pt, orc):
    """A condition on the inputs, asserted on the restatement."""
    classes, reasons = set(), set()
    for run in coverage_runs(pt, orc):
        for _, _, _, cls, dbg in run:
            classes |= set(np.unique(cls).tolist())
            reasons |= set(np.unique(dbg["taps"]).tolist())
    missing = [tr.CLASSES[k] for k in range(len(tr.CLASSES)) if k not in classes]
    assert not missing, missing
    missing = [name for k, name in tr.TAP_REASONS.items() if k not in reasons]
    assert not missing, missing
    assert tr.TAP_KEPT in reasons


# ---------------------------------------------------------------------------------------- properties
def test_constant_image_bit_for_bit(pt, orc):
    """A constant 0.5 comes back as 0.5 with length 1, 2, 3 where history was found: cur = 0.25 and every
    history colour is 0.25, so every wq * 0.25 is exact (scaling by a power of two commutes with rounding),
    ah = 0.25 * ws after every tap, h = 0.25, cur - h = 0 and sqrtf(0.25) = 0.5."""
    W, H = 7, 5
    frames = [(np.full((W * H, 3), F(0.5), F), aov, cam) for _, aov, cam in coherent_frames(pt, orc, W, H)]
    frames = [frames[0]] * 3   # a standing camera: every hit finds itself
    res = tr.sequence(frames, W, H, **OPTS)
    hit = frames[0][1]["obj"] >= 0
    assert hit.any() and (~hit).any()
    for call, (out, ln, _, _, _) in enumerate(res):
        np.testing.assert_array_equal(bits(out), bits(frames[0][0]))
        assert (ln[hit] == call + 1).all() and (ln[~hit] == 1).all()
    moving = tr.sequence([(np.full((W * H, 3), F(0.5), F), aov, cam) for _, aov, cam in coherent_frames(pt, orc, W, H)], W, H, **OPTS)
    for out, ln, _, _, _ in moving:
        np.testing.assert_array_equal(bits(out), bits(frames[0][0]))
    assert moving[2][1].max() > 2.0   # (fractional taps, lengths between 1 and 3)


def test_nan_history_contaminates_no_later_output(pt, orc):
    W, H = 37, 23
    frames = coherent_frames(pt, orc, W, H)
    bad0 = ~np.isfinite(frames[0][0]).all(1)
    assert bad0.sum() == 3
    res = tr.sequence(frames, W, H, **OPTS)
    assert (~np.isfinite(res[0][0]).all(1) == bad0).all()   # the first call has nothing to hide them with
    taps = res[1][4]["taps"]
    assert (taps == tr.TAP_NONFINITE).any()
    for out, ln, st, _, _ in res[1:]:
        assert np.isfinite(out).all() and np.isfinite(ln).all() and np.isfinite(st["hist"]["acc"]).all()


def test_max_history_one_turns_the_filter_off(pt, orc):
    """len = 1 everywhere and out = sqrtf(c * c) up to the blend's two roundings: with alpha = 1 the rule
    still evaluates h + (cur - h) * 1, and for colours in [0, 1] (cur, h and their difference within [-1, 1])
    the subtraction and the addition each round by at most 2^-25, so acc is within 2^-24 of c * c; out =
    sqrtf(acc) rounds by 2^-24 relative, its square by 2^-23 of acc <= 1 (and a term of 2^-48): out * out is
    within 2^-22 of c * c.  (out itself cannot be bounded absolutely: the root is steep at 0.)  Without
    history (the first call, misses) it is sqrtf(c * c) bit for bit."""
    W, H = 7, 5
    frames = adversarial_frames(pt, W, H, 5) + coherent_frames(pt, orc, W, H)
    blended = 0
    for (out, ln, st, cls, _), (rgb, _, _) in zip(tr.sequence(frames, W, H, **dict(OPTS, max_history=1.0)), frames):
        with np.errstate(all="ignore"):
            cur = rgb * rgb
            want = np.sqrt(cur)
        assert (ln == 1).all()
        finite = np.isfinite(rgb).all(1)
        assert np.abs(st["hist"]["acc"].reshape(-1, 3)[finite].astype(np.float64) - cur[finite]).max() <= 2.0 ** -24
        assert np.abs(out[finite].astype(np.float64) ** 2 - cur[finite]).max() <= 2.0 ** -22
        none = cls <= tr.ALL_TAPS_REJECTED
        blended += int((~none).sum())
        np.testing.assert_array_equal(bits(out[none]), bits(want[none]))
    assert blended > 0


def test_no_state_or_another_size_means_no_history(pt, orc):
    """The restatement's form of a reset is state=None (the library's is tested on the GPU): the call then
    is a first call, unlike the same call with the state; and a state of another frame size is not used."""
    W, H = 7, 5
    frames = coherent_frames(pt, orc, W, H)
    seq = tr.sequence(frames[:2], W, H, **OPTS)
    fresh = tr.temporal(*frames[1], None, W, H, **OPTS)
    assert (fresh[1] == 1).all() and (fresh[3] == tr.NO_HISTORY).all()
    assert seq[1][1].max() == 2.0 and (bits(seq[1][0]) != bits(fresh[0])).any()
    small = coherent_frames(pt, orc, 5, 3)[1]
    other_size = tr.temporal(*small, seq[0][2], 5, 3, **OPTS)
    assert (other_size[3] == tr.NO_HISTORY).all()
    np.testing.assert_array_equal(bits(other_size[0]), bits(tr.temporal(*small, None, 5, 3, **OPTS)[0]))


def test_miss_pixels_always_have_length_one(pt, orc):
    for run in coverage_runs(pt, orc)[:3]:
        for _, ln, st, cls, _ in run:
            miss = st["hist"]["hit"].reshape(-1) == 0
            assert miss.any() and (ln[miss] == 1).all()
            assert (cls[miss] <= tr.MISS).all()


def test_linear_skips_both_conversions(pt, orc):
    W, H = 7, 5
    frames = coherent_frames(pt, orc, W, H)
    lin = tr.sequence(frames, W, H, **dict(OPTS, linear=True))
    np.testing.assert_array_equal(bits(lin[0][0]), bits(frames[0][0]))   # first call: out = c, not sqrtf(c * c)
    sq = tr.sequence([(rgb * rgb, aov, cam) for rgb, aov, cam in frames], W, H, **dict(OPTS, linear=True))
    dflt = tr.sequence(frames, W, H, **OPTS)
    for (lo, ll_, ls, _, _), (do, dl, ds, _, _) in zip(sq, dflt):
        assert ls["hist"].tobytes() == ds["hist"].tobytes()   # the same history: a mean in linear radiance
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(bits(np.sqrt(lo)), bits(do))
        np.testing.assert_array_equal(bits(ll_), bits(dl))


# ------------------------------------------------------------------------------------------- quality
def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize("moving", [True, False], ids=["dolly", "standing"])
def test_history_is_closer_to_the_reference(pt, orc, moving):
    """Oracle frames (sample mode) of cornell at 48 x 48, depth 8, 1 spp: eight frames along a
    camera_move dolly (forward and to the right) or from a standing camera, against a 1024-spp frame of
    another seed at the last camera.  Temporal RMSE < the last noisy frame's; temporal then a-trous <
    a-trous alone (its colour tolerance from the frame's spp; after the history from spp x the mean
    history length of the hit pixels, the samples a pixel then stands for).  The ratios are printed and no
    tighter number is asserted: 0.213 (dolly of 11.2 units per frame) and 0.336 (standing; 1 / sqrt(8) =
    0.354 would be the linear-domain ideal) for the history, 0.378 for both of the second kind."""
    W = H = 48
    depth, spp, n_frames = 8, 1, 8
    p = pt.Preset("cornell", W, H)
    nodes = orc.build_lbvh(p.objects)
    rows = np.arange(H)
    cam = pt.Camera.from_buffer_copy(bytes(p.camera))
    state = None
    for f in range(n_frames):
        if moving and f:
            pt.camera_move(cam, 0, 4.0)   # FORWARD
            pt.camera_move(cam, 3, 2.0)   # RIGHT
        c = pt.camera_to_array(cam)
        noisy, _ = orc.render_sample(p.objects, p.materials, nodes, c, W, H, rows, spp, depth, seed=7 + f, nthreads=8)
        aov = atrous_ref.aov_ref(orc, p.objects, p.materials, c, W, H)
        out, ln, state, cls = tr.temporal(noisy, aov, c, state, W, H, **OPTS)
    ref, _ = orc.render_sample(p.objects, p.materials, nodes, c, W, H, rows, 1024, depth, seed=99, nthreads=8)
    hit = aov["obj"] >= 0
    found = float((cls[hit] >= tr.KEPT_PARTIAL).mean())
    mean_len = float(ln[hit].mean())
    den = atrous_ref.atrous(noisy, aov, W, H, iterations=5, sigma_color=atrous_ref.sigma_for(spp))
    both = atrous_ref.atrous(out, aov, W, H, iterations=5, sigma_color=atrous_ref.sigma_for(spp * mean_len))
    e_noisy, e_t, e_den, e_both = rmse(noisy, ref), rmse(out, ref), rmse(den, ref), rmse(both, ref)
    step = float(np.linalg.norm(c[:3] - pt.camera_to_array(p.camera)[:3])) / (n_frames - 1)
    print(f"cornell {W}x{H} {spp} spp, {'dolly' if moving else 'standing'} ({step:.3f} units per frame): noisy RMSE {e_noisy:.4f} "
          f"temporal {e_t:.4f} (ratio {e_t / e_noisy:.3f}), a-trous {e_den:.4f}, temporal + a-trous {e_both:.4f} "
          f"(ratio {e_both / e_den:.3f}); hit pixels with history {100 * found:.1f} %, mean length {mean_len:.2f}")
    assert e_t < e_noisy, (e_t, e_noisy)
    assert e_both < e_den, (e_both, e_den)
