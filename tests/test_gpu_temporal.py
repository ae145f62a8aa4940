"""pt_film_temporal on the GPU: every call of a sequence bit for bit against the numpy restatement
(tests/temporal_ref.py, itself held to a per-pixel loop by tests/test_temporal_host.py) -- `out`, `out_len`
and, through the later calls, the stored history -- on synthetic and real guides, host and device
pointers, in place, enqueued in front of pt_film_denoise, refused calls, resets, and what the call must
leave alone.
"""
import numpy as np
import pytest
import torch  # before libpt.so loads (the two must share torch's HIP runtime)

import atrous_ref
import temporal_ref as tr
from atrous_ref import lit_soup

pytestmark = pytest.mark.gpu
PT_ERR_INVALID = 1
ADV = dict(sigma_plane=0.05, normal_cos=0.5)   # (the options the host tests' coverage condition is asserted with)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def camera(pt, words):
    return pt.Camera.from_buffer_copy(np.asarray(words, np.float32).tobytes())


@pytest.fixture(scope="module")
def refs(pt, orc):
    """The restatement's three-call sequence of each (kind, W, H, opts) once: (frames, results)."""
    cache = {}

    def get(kind, W, H, **opts):
        key = (kind, W, H, tuple(sorted(opts.items())))
        if key not in cache:
            frames = tr.coherent_frames(pt, orc, W, H) if kind == "coherent" else tr.adversarial_frames(pt, W, H, 3)
            cache[key] = (frames, tr.sequence(frames, W, H, **opts))
        return cache[key]
    return get


def check_sequence(pt, film, frames, want, first=0, **opts):
    for call in range(first, len(frames)):
        rgb, aov, cam = frames[call]
        keep = rgb.copy()
        out, ln = pt.temporal(film, rgb, aov, camera(pt, cam), **opts)
        same_bits(out, want[call][0], f"out of call {call}")
        same_bits(ln, want[call][1], f"out_len of call {call}")
        same_bits(rgb, keep, "the input")


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (37, 23), (70, 45), (130, 9)])
def test_sizes_synthetic_guides(pt, gpu, refs, W, H):
    """1 x 1; 70 x 45 across every 32 x 8 tile edge; a wide, low frame.  Three calls on one film with three
    cameras; NaN and inf pixels wherever the frame has room for them."""
    frames, want = refs("adversarial", W, H, **ADV)
    check_sequence(pt, pt.Film(W, H, 1, device=gpu), frames, want, **ADV)
    if W * H > 2 * W + 2:
        assert not np.isfinite(want[0][0]).all()


@pytest.mark.parametrize("max_history", [1.0, 2.0])
@pytest.mark.parametrize("kind", ["coherent", "adversarial"])
def test_max_history(pt, gpu, refs, kind, max_history):
    W, H = 37, 23
    opts = dict(ADV, max_history=max_history) if kind == "adversarial" else dict(max_history=max_history)
    frames, want = refs(kind, W, H, **opts)
    check_sequence(pt, pt.Film(W, H, 1, device=gpu), frames, want, **opts)
    assert want[2][1].max() == max_history


def test_linear_flag(pt, gpu, refs):
    W, H = 37, 23
    frames, want = refs("coherent", W, H, linear=True)
    check_sequence(pt, pt.Film(W, H, 1, device=gpu), frames, want, linear=True)


def test_real_guides(pt, gpu):
    """pt.render (2 spp, depth 6) and pt.render_aov of the soup from three cameras, through host pointers."""
    objs, mats = lit_soup()
    W, H = 37, 23
    scene = pt.Scene(objs, mats, device=gpu)
    film = pt.Film(W, H, 4, device=gpu)
    state = None
    for call, cam in enumerate(tr.soup_cameras(pt, W, H)):
        rgb, _ = pt.render(scene, film, cam, 2, 6)
        aov, _ = pt.render_aov(scene, film, cam)
        want_out, want_len, state, cls = tr.temporal(rgb, aov, pt.camera_to_array(cam), state, W, H)
        hit = aov["obj"] >= 0
        if call:   # a condition on the cameras, checked on the restatement
            assert (cls[hit] >= tr.KEPT_PARTIAL).sum() * 2 > hit.sum()
        out, ln = pt.temporal(film, rgb, aov, cam)
        same_bits(out, want_out, f"out of call {call}")
        same_bits(ln, want_len, f"out_len of call {call}")
        if call:
            assert (out != rgb).any() and ln.max() == call + 1


def dev(t):
    return t.data_ptr()


def to_dev(a, device):
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(device)


def floats(t, cols=3):
    return np.frombuffer(t.cpu().numpy().tobytes(), np.float32).reshape(-1, cols)


def test_device_pointers_in_place_and_no_length(pt, gpu, refs):
    """Device pointers give the host pointers' bits; the inputs are left alone when out != rgb; out == rgb
    works; out_len == NULL works (the history it would have reported shows in the next call)."""
    W, H = 37, 23
    frames, want = refs("adversarial", W, H, **ADV)
    d = torch.device("cuda", gpu)
    film = pt.Film(W, H, 1, device=gpu)
    for call, (rgb, aov, cam) in enumerate(frames):
        dc, dg = to_dev(rgb, d), to_dev(aov, d)
        out = torch.zeros_like(dc)
        ln = torch.zeros(W * H, dtype=torch.float32, device=d)
        torch.cuda.synchronize(d)
        if call == 0:     # separate output, with lengths
            assert pt.temporal(film, dev(dc), dev(dg), camera(pt, cam), out=dev(out), out_len=dev(ln), **ADV) is None
            torch.cuda.synchronize(d)
            same_bits(floats(out), want[call][0])
            same_bits(floats(ln, 1), want[call][1])
            same_bits(floats(dc), rgb)
            assert dg.cpu().numpy().tobytes() == aov.tobytes()
        elif call == 1:   # in place, no lengths
            pt.temporal(film, dev(dc), dev(dg), camera(pt, cam), **ADV)
            torch.cuda.synchronize(d)
            same_bits(floats(dc), want[call][0])
        else:             # in place, given explicitly, with lengths
            pt.temporal(film, dev(dc), dev(dg), camera(pt, cam), out=dev(dc), out_len=dev(ln), **ADV)
            torch.cuda.synchronize(d)
            same_bits(floats(dc), want[call][0])
            same_bits(floats(ln, 1), want[call][1])
    host = frames[0][0].copy()
    fresh = pt.Film(W, H, 1, device=gpu)
    out, _ = pt.temporal(fresh, host, frames[0][1], camera(pt, frames[0][2]), out=host, **ADV)
    assert out is host
    same_bits(host, want[0][0])


def test_three_calls_then_denoise_on_one_stream(pt, gpu, refs):
    """Enqueued back to back on a non-default stream, nothing waited for in between: the history images take
    turns at enqueue time, and the a-trous passes' scratch images are not theirs."""
    W, H = 70, 45
    frames, want = refs("adversarial", W, H, **ADV)
    dn = dict(iterations=5, sigma_color=0.6, sigma_albedo=0.1, sigma_plane=0.02)
    d = torch.device("cuda", gpu)
    stream = torch.cuda.Stream(d)
    film = pt.Film(W, H, 1, device=gpu)
    dc = [to_dev(f[0], d) for f in frames]
    dg = [to_dev(f[1], d) for f in frames]
    outs = [torch.zeros_like(c) for c in dc]
    lens = [torch.zeros(W * H, dtype=torch.float32, device=d) for _ in frames]
    den = torch.zeros_like(dc[0])
    torch.cuda.synchronize(d)
    for i, f in enumerate(frames):
        pt.temporal(film, dev(dc[i]), dev(dg[i]), camera(pt, f[2]), out=dev(outs[i]), out_len=dev(lens[i]),
                    stream=stream.cuda_stream, **ADV)
    pt.denoise(film, dev(outs[2]), dev(dg[2]), out=dev(den), stream=stream.cuda_stream, **dn)
    stream.synchronize()
    for i in range(3):
        same_bits(floats(outs[i]), want[i][0], f"out of call {i}")
        same_bits(floats(lens[i], 1), want[i][1], f"out_len of call {i}")
    same_bits(floats(den), atrous_ref.atrous(want[2][0], frames[2][1], W, H, **dn))


BAD_OPTS = [dict(max_history=0.5), dict(max_history=float("nan")), dict(sigma_plane=0.0), dict(sigma_plane=float("inf")),
            dict(normal_cos=1.5), dict(normal_cos=float("nan"))]


def test_refused_calls_leave_no_trace(pt, gpu, refs):
    """Invalid options between two valid calls: PT_ERR_INVALID, `out` and `out_len` keep their sentinel, and
    the next valid call is the sequence's next one."""
    W, H = 37, 23
    frames, want = refs("adversarial", W, H, **ADV)
    film = pt.Film(W, H, 1, device=gpu)
    check_sequence(pt, film, frames[:1], want, **ADV)
    rgb, aov, cam = frames[1]
    for bad in BAD_OPTS:
        out, ln = np.full((W * H, 3), 7.0, np.float32), np.full(W * H, 7.0, np.float32)
        with pytest.raises(pt.PtError) as e:
            pt.temporal(film, rgb.copy(), aov, camera(pt, cam), out=out, out_len=ln, **dict(ADV, **bad))
        assert e.value.code == PT_ERR_INVALID and list(bad)[0] in str(e.value)
        assert (out == 7.0).all() and (ln == 7.0).all()
    check_sequence(pt, film, frames, want, first=1, **ADV)


def test_partitioned_film_is_refused(pt, gpu, refs):
    W, H = 37, 23
    frames, _ = refs("adversarial", W, H, **ADV)
    film = pt.Film(W, H, 1, device=gpu, stripe_height=8, n_parts=2, part=0)
    n = film.n_pixels
    out, ln = np.full((n, 3), 7.0, np.float32), np.full(n, 7.0, np.float32)
    with pytest.raises(pt.PtError) as e:
        pt.temporal(film, frames[0][0][:n].copy(), frames[0][1][:n].copy(), camera(pt, frames[0][2]), out=out, out_len=ln)
    assert e.value.code == PT_ERR_INVALID and "n_parts" in str(e.value)
    assert (out == 7.0).all() and (ln == 7.0).all()


def test_reset_starts_a_new_history(pt, gpu, refs, orc):
    W, H = 37, 23
    frames, want = refs("coherent", W, H)
    film = pt.Film(W, H, 1, device=gpu)
    check_sequence(pt, film, frames[:2], want)
    assert want[1][1].max() == 2.0
    film.temporal_reset()
    # what a fresh film computes for frames 2, then 1: the restatement from no state
    a = tr.temporal(*frames[2], None, W, H)
    b = tr.temporal(*frames[1], a[2], W, H)
    for (rgb, aov, cam), ref in ((frames[2], a), (frames[1], b)):
        out, ln = pt.temporal(film, rgb, aov, camera(pt, cam))
        same_bits(out, ref[0])
        same_bits(ln, ref[1])
    assert (a[1] == 1).all() and b[1].max() == 2.0
    fresh = pt.Film(W, H, 1, device=gpu)
    out, ln = pt.temporal(fresh, frames[2][0], frames[2][1], camera(pt, frames[2][2]))
    same_bits(out, a[0])


def test_the_film_is_otherwise_untouched(pt, gpu, refs):
    """The streams, the accumulated sums and a following frame are those of a film that never made a temporal
    call; the history in turn survives pt_film_clear and pt_film_reset."""
    objs, mats = lit_soup()
    W, H = 37, 23
    frames, want = refs("coherent", W, H)
    scene = pt.Scene(objs, mats, device=gpu)
    cam = tr.soup_cameras(pt, W, H)[0]
    films = [pt.Film(W, H, 9, device=gpu) for _ in range(2)]
    first = [pt.render(scene, f, cam, 2, 6, rng=pt.RNG_SAMPLE, accumulate=True)[0] for f in films]
    same_bits(first[0], first[1])
    check_sequence(pt, films[0], frames[:2], want)
    assert films[0].accumulated == films[1].accumulated == 2
    np.testing.assert_array_equal(films[0].get_rng(), films[1].get_rng())
    second = [pt.render(scene, f, cam, 2, 6, rng=pt.RNG_SAMPLE, accumulate=True)[0] for f in films]
    same_bits(second[0], second[1])
    assert films[0].accumulated == 4
    films[0].clear()
    films[0].reset()
    check_sequence(pt, films[0], frames, want, first=2)
