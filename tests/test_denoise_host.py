"""pt_film_denoise's rule on the CPU: the numpy restatement (tests/atrous_ref.py, what the GPU tests
hold the kernel to bit for bit) against a plain per-pixel loop that follows include/pt.h line by
line, the filter's invariants, and the condition that it helps at all: on low-spp frames of the
oracle the denoised frame is closer to a 1024-spp frame than the noisy one.
"""
import numpy as np
import pytest

import atrous_ref
from atrous_ref import F, synthetic_guides, synthetic_image

K = (F(0.375), F(0.25), F(0.0625))


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def loop_pass(c, g, step, isa2, isc2, sp):
    """include/pt.h's pass, pixel by pixel and tap by tap, in np.float32 scalars."""
    H, W = g.shape
    out = np.zeros((H, W, 3), F)
    for y in range(H):
        for x in range(W):
            P = g[y, x]
            hit_p = P["obj"] >= 0
            acc = [F(0), F(0), F(0)]
            ws = F(0)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = x + dx * step, y + dy * step
                    if qx < 0 or qx >= W or qy < 0 or qy >= H:
                        continue
                    h = K[abs(dx)] * K[abs(dy)]
                    if dx == 0 and dy == 0:
                        w = h
                    else:
                        Q = g[qy, qx]
                        if (Q["obj"] >= 0) != hit_p:
                            continue
                        if hit_p:
                            wn = F(np.fmax(F(0), dot(P["n"], Q["n"])))
                            for _ in range(6):
                                wn = wn * wn
                            dp = Q["p"] - P["p"]
                            dist = np.abs(dot(P["n"], dp))
                            xx = dist / (F(sp) * P["depth"])
                            wp = F(1) / (F(1) + xx * xx)
                        else:
                            wn = wp = F(1)
                        da = Q["albedo"] - P["albedo"]
                        wa = F(1) / (F(1) + dot(da, da) * isa2)
                        dc = c[qy, qx] - c[y, x]
                        wc = F(1) / (F(1) + dot(dc, dc) * isc2)
                        w = (((h * wn) * wp) * wa) * wc
                    if not w > 0:
                        continue
                    for ch in range(3):
                        acc[ch] = acc[ch] + w * c[qy, qx, ch]
                    ws = ws + w
            for ch in range(3):
                out[y, x, ch] = acc[ch] / ws
    return out


def loop_atrous(rgb, aov, W, H, iterations, sigma_color, sigma_albedo, sigma_plane):
    c = np.asarray(rgb, F).reshape(H, W, 3).copy()
    g = aov.reshape(H, W)
    with np.errstate(all="ignore"):
        isa2 = F(1) / (F(sigma_albedo) * F(sigma_albedo))
        for i in range(iterations):
            sc = F(sigma_color) * (F(1) / F(1 << i))
            c = loop_pass(c, g, 1 << i, isa2, F(1) / (sc * sc), sigma_plane)
    return c.reshape(-1, 3)


CASES = [(7, 5, 3, 5), (5, 3, 4, 3), (7, 5, 5, 1)]


@pytest.mark.parametrize("W,H,seed,iters", CASES)
def test_restatement_equals_loop(W, H, seed, iters):
    g = synthetic_guides(W, H, seed)
    c = synthetic_image(W, H, seed)
    kw = dict(iterations=iters, sigma_color=0.6, sigma_albedo=0.1, sigma_plane=0.02)
    a = atrous_ref.atrous(c, g, W, H, **kw)
    b = loop_atrous(c, g, W, H, **kw)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(a).any() and not np.isfinite(a).all()


def test_normal_weight_passes_through_the_denormals():
    wn = F(0.2)
    for _ in range(6):
        wn = wn * wn
    assert 0 < wn < np.finfo(F).tiny


def test_constant_image_bit_for_bit():
    """A constant image comes back bit for bit, whatever the guides: with the value v a power of two
    every w * v is exact, so acc = v * ws holds after every tap and acc / ws is v.  (For another v each
    pass rounds 25 products, 2 x 25 additions and a division, at most 2^-24 each, and averages what
    the passes before it left: within 5 x 76 x 2^-24.)"""
    W, H = 7, 5
    g = synthetic_guides(W, H, 9)
    c = np.full((W * H, 3), F(0.25), F)
    out = atrous_ref.atrous(c, g, W, H, **atrous_ref.DEFAULTS)
    np.testing.assert_array_equal(out.view(np.uint32), c.view(np.uint32))
    c = np.full((W * H, 3), F(0.37), F)
    out = atrous_ref.atrous(c, g, W, H, **atrous_ref.DEFAULTS)
    np.testing.assert_allclose(out, c, rtol=5 * 76 * 2.0 ** -24, atol=0)


def test_zero_iterations_is_a_copy():
    W, H = 7, 5
    img = synthetic_image(W, H, 9)
    same = atrous_ref.atrous(img, synthetic_guides(W, H, 9), W, H, iterations=0)
    np.testing.assert_array_equal(same.view(np.uint32), img.view(np.uint32))


def test_hit_and_miss_do_not_mix():
    W, H = 7, 5
    g = synthetic_guides(W, H, 5)
    miss = g["obj"] < 0
    assert miss.any() and (~miss).any()
    c = np.where(miss[:, None], F(2.0), F(0.5)).astype(F) * np.ones((1, 3), F)
    out = atrous_ref.atrous(c, g, W, H, **atrous_ref.DEFAULTS)
    np.testing.assert_allclose(out[miss], 2.0, rtol=1e-6)
    np.testing.assert_allclose(out[~miss], 0.5, rtol=1e-6)


def test_nan_only_where_the_centre_is():
    """A NaN or inf pixel poisons no neighbour (its taps have w = NaN or 0 and are skipped); it stays
    itself: the centre tap is always kept, and inf's own other taps are skipped (dc = -inf, wc = 0)."""
    W, H = 7, 5
    g = synthetic_guides(W, H, 6)
    c = synthetic_image(W, H, 6)
    out = atrous_ref.atrous(c, g, W, H, **atrous_ref.DEFAULTS)
    nan_in = np.isnan(c).any(1)
    np.testing.assert_array_equal(np.isnan(out).any(1), nan_in)
    inf_in = np.isinf(c).any(1)
    np.testing.assert_array_equal(np.isinf(out).any(1), inf_in)
    assert np.isfinite(out[~nan_in & ~inf_in]).all()


# ------------------------------------------------------------------------------------------ quality
def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


QUALITY = [("cornell", 48, 48, 8, (1, 4, 16)), ("bunny_cornell", 64, 36, 12, (1, 4, 16)), ("rtiow", 60, 40, 0, (1, 4))]


@pytest.mark.parametrize("name,W,H,depth,counts", QUALITY, ids=[q[0] for q in QUALITY])
def test_denoised_frame_is_closer_to_the_reference(pt, orc, name, W, H, depth, counts):
    """Oracle frames (sample mode) at 1 / 4 / 16 spp against a 1024-spp frame of another film seed,
    sigma_color = 1.2 / sqrt(spp), 5 passes: denoised RMSE < noisy RMSE.  rtiow at 16 spp is not
    asserted: its glass and metal show detail that first-hit guides do not see, and the prototype
    sat at a ratio of 0.99 there."""
    p = pt.Preset(name, W, H)
    depth = depth or p.max_depth
    cam = pt.camera_to_array(p.camera)
    nodes = orc.build_lbvh(p.objects)
    rows = np.arange(H)
    ref, _ = orc.render_sample(p.objects, p.materials, nodes, cam, W, H, rows, 1024, depth, seed=99, nthreads=8)
    aov = atrous_ref.aov_ref(orc, p.objects, p.materials, cam, W, H)
    for spp in counts:
        noisy, _ = orc.render_sample(p.objects, p.materials, nodes, cam, W, H, rows, spp, depth, seed=7, nthreads=8)
        den = atrous_ref.atrous(noisy, aov, W, H, iterations=5, sigma_color=atrous_ref.sigma_for(spp))
        e_noisy, e_den = rmse(noisy, ref), rmse(den, ref)
        print(f"{name} {W}x{H} {spp} spp: noisy RMSE {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
        assert e_den < e_noisy, (name, spp, e_noisy, e_den)
