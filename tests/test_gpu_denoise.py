"""pt_film_denoise on the GPU: the a-trous passes bit for bit against the numpy restatement
(tests/atrous_ref.py, itself held to a per-pixel loop by tests/test_denoise_host.py), on real and
synthetic guides, every iteration count, host and device pointers, in place, enqueued, and through
the command-line app.
"""
import os
import subprocess

import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

import atrous_ref
from atrous_ref import lit_soup, synthetic_guides, synthetic_image
from helpers import read_png

pytestmark = pytest.mark.gpu
PT_ERR_INVALID = 1
OPTS = dict(iterations=5, sigma_color=0.6, sigma_albedo=0.1, sigma_plane=0.02)


def same_bits(got, want):
    np.testing.assert_array_equal(np.asarray(got).reshape(-1, 3).view(np.uint32), np.asarray(want).reshape(-1, 3).view(np.uint32))


@pytest.fixture(scope="module")
def refs():
    """The restatement of each (W, H, seed, special, opts) once."""
    cache = {}

    def get(W, H, seed, special=True, **opts):
        key = (W, H, seed, special, tuple(sorted(opts.items())))
        if key not in cache:
            g, c = synthetic_guides(W, H, seed), synthetic_image(W, H, seed, special)
            cache[key] = (g, c, atrous_ref.atrous(c, g, W, H, **opts))
        g, c, want = cache[key]
        return g.copy(), c.copy(), want
    return get


@pytest.mark.parametrize("W,H,iters", [(1, 1, 5), (5, 3, 5), (37, 23, 5), (70, 45, 6), (130, 9, 5)])
def test_sizes_synthetic_guides(pt, gpu, refs, W, H, iters):
    """1 x 1; 37 x 23 with the fifth pass's reach of 32 beyond the frame; 70 x 45 with 6 passes, across
    every 16-, 32- and 64-wide tile edge; a wide, low frame.  NaN and inf pixels included."""
    opts = dict(OPTS, iterations=iters)
    special = W * H > 2 * W + 2
    g, c, want = refs(W, H, 3, special, **opts)
    got = pt.denoise(pt.Film(W, H, 1, device=gpu), c, g, **opts)
    same_bits(got, want)
    assert special == bool(np.isnan(want).any())


def test_real_guides(pt, gpu):
    """render_aov's guides of the soup with a rendered 2-spp frame (host pointers), default sigma from spp."""
    objs, mats = lit_soup()
    W, H = 37, 23
    scene = pt.Scene(objs, mats, device=gpu)
    film = pt.Film(W, H, 4, device=gpu)
    cam = pt.camera_make((0, 0, 28), (0, 0, 0), 50, W / H)
    rgb, _ = pt.render(scene, film, cam, 2, 6)
    aov, _ = pt.render_aov(scene, film, cam)
    got = pt.denoise(film, rgb, aov, spp=2)
    want = atrous_ref.atrous(rgb, aov, W, H, iterations=5, sigma_color=float(np.float32(atrous_ref.sigma_for(2))))
    same_bits(got, want)
    assert (got != rgb).any()


@pytest.mark.parametrize("iters", range(9))
def test_iterations(pt, gpu, refs, iters):
    W, H = 37, 23
    opts = dict(OPTS, iterations=iters)
    g, c, want = refs(W, H, 4, True, **opts)
    same_bits(pt.denoise(pt.Film(W, H, 1, device=gpu), c, g, **opts), want)
    if iters == 0:
        same_bits(want, c)


def dev(t):
    return t.data_ptr()


def to_dev(a, device):
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(device)


def floats(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), np.float32).reshape(-1, 3)


@pytest.mark.parametrize("iters", [1, 2, 5])
def test_device_pointers_and_in_place(pt, gpu, refs, iters):
    """Device pointers give the host pointers' bits; out == rgb works (1 pass: through a scratch image)."""
    W, H = 37, 23
    opts = dict(OPTS, iterations=iters)
    g, c, want = refs(W, H, 4, True, **opts)
    d = torch.device("cuda", gpu)
    film = pt.Film(W, H, 1, device=gpu)
    dc, dg = to_dev(c, d), to_dev(g, d)
    out = torch.zeros_like(dc)
    torch.cuda.synchronize(d)
    assert pt.denoise(film, dev(dc), dev(dg), out=dev(out), **opts) is None
    torch.cuda.synchronize(d)
    same_bits(floats(out), want)
    same_bits(floats(dc), c)   # the input is left alone
    pt.denoise(film, dev(dc), dev(dg), out=dev(dc), **opts)
    torch.cuda.synchronize(d)
    same_bits(floats(dc), want)
    host = c.copy()
    assert pt.denoise(film, host, g, out=host, **opts) is host
    same_bits(host, want)


def test_two_calls_back_to_back_on_one_stream(pt, gpu, refs):
    W, H = 70, 45
    a, b = dict(OPTS, iterations=6), dict(OPTS, iterations=3, sigma_color=0.3, sigma_plane=0.05)
    g, c, want_a = refs(W, H, 3, True, **a)
    _, _, want_b = refs(W, H, 3, True, **b)
    d = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(d)
    film = pt.Film(W, H, 1, device=gpu)
    dc, dg = to_dev(c, d), to_dev(g, d)
    oa, ob = torch.zeros_like(dc), torch.zeros_like(dc)
    torch.cuda.synchronize(d)
    pt.denoise(film, dev(dc), dev(dg), out=dev(oa), stream=stream.cuda_stream, **a)
    pt.denoise(film, dev(dc), dev(dg), out=dev(ob), stream=stream.cuda_stream, **b)
    stream.synchronize()
    same_bits(floats(oa), want_a)
    same_bits(floats(ob), want_b)
    # a second call on the same film: the same bits (the scratch images are reused)
    pt.denoise(film, dev(dc), dev(dg), out=dev(ob), stream=stream.cuda_stream, **a)
    stream.synchronize()
    same_bits(floats(ob), want_a)


def test_partitioned_film_is_refused(pt, gpu, refs):
    W, H = 37, 23
    g, c, _ = refs(W, H, 4, True, **OPTS)
    film = pt.Film(W, H, 1, device=gpu, stripe_height=8, n_parts=2, part=0)
    n = film.n_pixels
    out = np.full((n, 3), 7.0, np.float32)
    with pytest.raises(pt.PtError) as e:
        pt.denoise(film, c[:n].copy(), g[:n].copy(), out=out, **OPTS)
    assert e.value.code == PT_ERR_INVALID and "n_parts" in str(e.value)
    assert (out == 7.0).all()


def test_app_denoise_flag(pt, gpu, tmp_path):
    """pt_render_png --denoise writes the PNG that quantize_png of the restatement gives; with more
    than one GPU it is refused with the usage text."""
    import oracle
    app = os.path.join(pt.PKG, "pt_render_png")
    W = H = 48
    out = tmp_path / "d.png"
    r = subprocess.run([app, "--scene", "cornell_lit", "--models", pt.MODELS_DIR, "--width", str(W), "--height", str(H),
                        "--spp", "4", "--mis", "--denoise", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    p = pt.Preset("cornell_lit", W, H)
    scene = pt.Scene(p.objects, p.materials, device=gpu)
    scene.set_sky(*p.sky)
    film = pt.Film(W, H, 1, device=gpu)
    rgb, _ = pt.render(scene, film, p.camera, 4, p.max_depth, mis=True)
    aov, _ = pt.render_aov(scene, film, p.camera)
    want = atrous_ref.atrous(rgb, aov, W, H, iterations=5, sigma_color=float(np.float32(atrous_ref.sigma_for(4))))
    png = read_png(str(out))
    np.testing.assert_array_equal(png, oracle.quantize_png(want).reshape(H, W, 4)[::-1])
    assert (png != oracle.quantize_png(rgb).reshape(H, W, 4)[::-1]).any()
    # with --frames and --nee: the tolerance comes from the accumulated sample count unless it is given
    common = [app, "--scene", "cornell_lit", "--models", pt.MODELS_DIR, "--width", "24", "--height", "24", "--spp", "2",
              "--frames", "2", "--nee", "--denoise", "--out", str(tmp_path / "f.png")]
    r = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "denoised: 4 spp, sigma_color 0.6000" in r.stdout, r.stdout + r.stderr
    r = subprocess.run(common + ["--denoise-sigma", "0.25"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "denoised: 4 spp, sigma_color 0.2500" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([app, "--scene", "cornell_lit", "--models", pt.MODELS_DIR, "--gpus", "2", "--denoise",
                        "--out", str(tmp_path / "no.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage:" in r.stderr
    assert not os.path.exists(tmp_path / "no.png")
