"""The polarisation view of a Stokes film on the MI355X (wtgpu_film_polar_device; csrc/kernels_polar.hip) against the host twin, bit for bit: the
four counts, max_dop and argmax, the six sums, all six maps — the two angles among them, since neither side calls a libm function
(wt/film_polar.h) — and the picture with the linear operator; the sRGB / gamma / dB pictures within one code.  The host twin itself is held to
a numpy restatement by tests/test_film_polar.py, whose films are used here: P = 4 and 12 planes at 37 x 23 (851 pixels: a part of one block,
chunks that end inside the film) and at 256 x 192 (192 chunks: 48 blocks, a second level of chunk sums); P = 12 at 257 x 256 (257 chunks, then 2,
then 1: the reduction's loop runs twice).  Then rendered films, and what the calls leave alone."""
import ctypes as C

import numpy as np
import pytest

from test_film_polar import DERIVED, EARLY, FIELDS, LATE, MAPS, NO_PIXEL, PICTURE_TMS, POLAR, SPE, THETA, late_tie_films, polar_films
from test_film_stats import F32, LEVELS, checker, same_bits, stats_scene
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (256, 192)]


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_film_polar")
    return {(w, h, P): stats_scene(d, P, w, h).upload(0) for w, h in SIZES + [LEVELS] for P in (sorted(POLAR) if (w, h) != LEVELS else (12,))}


def _same(sc, films, d_films, mask, d_mask, label, **kw):
    got = sc.film_polar_device(*d_films, SPE, mask=d_mask, maps=MAPS, **kw)
    want = sc.film_polar_host(*films, SPE, mask=mask, maps=MAPS, threads=16, **kw)
    for k in FIELDS + DERIVED:
        assert same_bits(got[k], want[k]), (label, kw, k, got[k], want[k])
    for k in MAPS:
        assert same_bits(got["maps"][k].cpu().numpy(), want["maps"][k]), (label, kw, k)
    if kw.get("picture"):
        g = got["picture"].cpu().numpy()
        g = g.view(np.uint16) if kw.get("fmt") == "u16" else g
        assert g.dtype == want["picture"].dtype and same_bits(g, want["picture"]), (label, kw, "picture")
    return got


def _one_film(scenes, size, P, seed):
    W, H = size
    sc = scenes[(W, H, P)]
    channels = POLAR[P]
    films = polar_films(H, W, channels, seed)
    d_films = _to_device(sc, films)
    mask = checker(H, W)
    d_mask, = _to_device(sc, (mask,))
    fmts = ("f32", "u8", "u16")
    k = 0
    for lum in ((False, True) if channels == 3 else (False,)):
        for masked in (False, True):
            for plane in range(channels + lum):
                k += 1
                got = _same(sc, films, d_films, mask if masked else None, d_mask if masked else None, (size, P), luminance=lum, analyser=THETA, picture=True,
                            picture_plane=plane, fmt=fmts[k % 3], sat_gain=(1.0, 2.5)[k % 2])
                assert got["n"][0] == (int((mask > 0).sum()) if masked else W * H) and got["picture"].shape == (H, W, 4 if masked else 3)
                assert got["n_nonfinite"].all() and got["n_dark"].all() and got["n_over"].all() and (got["argmax"] < W * H).all() and (got["sum_pol"] > 0).all()
    # no maps, no picture: the records alone
    bare = sc.film_polar_device(*d_films, SPE, luminance=channels == 3)
    assert bare["maps"] == {} and bare["picture"] is None
    assert all(same_bits(bare[f], sc.film_polar_host(*films, SPE, luminance=channels == 3)[f]) for f in FIELDS)
    # the operators that call libm: within one code of the host twin
    for tm in PICTURE_TMS:
        for fmt in ("u8", "u16"):
            kw = dict(luminance=channels == 3, picture=True, picture_plane=channels - 1, tm=tm, fmt=fmt, sat_gain=1.5)
            g = sc.film_polar_device(*d_films, SPE, mask=d_mask, **kw)["picture"].cpu().numpy()
            g = (g.view(np.uint16) if fmt == "u16" else g).astype(np.int64)
            h = sc.film_polar_host(*films, SPE, mask=mask, **kw)["picture"].astype(np.int64)
            assert g.shape == h.shape and np.abs(g - h).max() <= 1 and np.array_equal(g[..., 3], h[..., 3]), (size, P, tm, fmt)


@pytest.mark.parametrize("P", sorted(POLAR))
def test_device_equals_host_twin(scenes, P):
    _one_film(scenes, SIZES[0], P, 100 + P)


@pytest.mark.parametrize("P", sorted(POLAR))
def test_device_equals_host_twin_on_many_chunks(scenes, P):
    _one_film(scenes, SIZES[1], P, 200 + P)


def test_device_equals_host_twin_over_two_levels(scenes):
    """257 x 256: k_film_finish goes round its loop twice, the second time over what the first wrote."""
    _one_film(scenes, LEVELS, 12, 312)


def test_a_late_maximum_and_a_tie_across_the_wavefronts_records(scenes):
    """257 x 256: 257 chunks on 65 blocks, 260 wavefront records — k_film_finish's 256 threads go round the records twice.  The maximum is in the
    last chunk (record 256, the second round) with its equal in chunk 3 (record 3): argmax is the smaller pixel; without the early one, the late."""
    sc = scenes[LEVELS + (12,)]
    for early in (True, False):
        films = late_tie_films(early)
        got = _same(sc, films, _to_device(sc, films), None, None, ("late tie", early))
        assert got["argmax"].tolist() == [(EARLY if early else LATE) + c for c in range(3)] and got["max_dop"].tolist() == [0.75] * 3


def test_the_measured_alternative_computes_the_same(built, tmp_path, monkeypatch):
    """The form the A/B of csrc/kernels_polar.hip left behind its knob — every lane loads the planes of its own pixels, no LDS — gives the default
    form's bits: a part of one block (chunks that end inside the film), and the 257 chunks of the two-level film."""
    monkeypatch.setenv("WTGPU_FILM_POLAR_STAGED", "0")
    for (W, H), P in ((SIZES[0], 4), (SIZES[0], 12), (LEVELS, 12)):
        sc = stats_scene(tmp_path, P, W, H).upload(0)
        films = polar_films(H, W, POLAR[P], 7)
        mask = checker(H, W)
        for lum in ((False, True) if P == 12 else (False,)):
            got = _same(sc, films, _to_device(sc, films), mask, _to_device(sc, (mask,))[0], ("per lane", W, H, P), luminance=lum, analyser=THETA, picture=True,
                        picture_plane=POLAR[P] - 1 + lum, fmt="u16", sat_gain=2.0)
            assert got["n_nonfinite"].all() and got["n_dark"].all() and got["n_over"].all()


def test_a_mask_that_excludes_everything(scenes):
    for W, H in SIZES:
        sc = scenes[(W, H, 12)]
        films = polar_films(H, W, 3, 5)
        mask = np.zeros((H, W), F32)
        mask[0, 0] = np.nan
        got = _same(sc, films, _to_device(sc, films), mask, _to_device(sc, (mask,))[0], (W, H), luminance=True, picture=True, fmt="u8")
        assert not got["n"].any() and not got["sum_i"].any() and (got["argmax"] == NO_PIXEL).all() and not any(m.any() for m in got["maps"].values())
        assert got["picture"][..., :3].any() and not got["picture"][..., 3].any()      # every pixel is shown; the mask is the alpha


def test_rendered_films(built):
    """cornell_box polarimetric on the device: device = host twin on the downloaded films, and render.polarisation gives the same from the torch
    films as from the numpy ones."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films, polarisation
    dev = torch.device("cuda", 0)
    sc = Scene("cornell_box", polarimetric=1, res=24, mesh_detail=0, crop_of=1440, lut=(64, 64)).upload(0)
    d_films = alloc_films(sc, dev)
    sc.render_into(*d_films, 0, 8, 3, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    films = tuple(t.cpu().numpy() for t in d_films)
    got = _same(sc, films, d_films, None, None, "cornell_box", luminance=True, analyser=THETA, picture=True, picture_plane=3, fmt="u8", sat_gain=2.0)
    assert (got["mean_dolp"] > 0).all() and not got["n_nonfinite"].any() and (got["n"] == sc.width * sc.height).all() and got["picture"].any()
    a, b = polarisation(sc, d_films, 8, luminance=True), polarisation(sc, films, 8, luminance=True)
    assert all(same_bits(a[k], b[k]) for k in FIELDS + DERIVED)


def test_polar_between_renders_changes_nothing(built):
    """As test_gpu_film_compare.py::test_compare_between_renders_changes_nothing: the call counts nothing and leaves the films it reads alone."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", polarimetric=1, res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_a = _to_device(sc, a)
    got = sc.film_polar_device(*d_a, 2, luminance=sc.spectral_channels == 3, maps=MAPS, picture=True)
    assert all(v == 0 for v in sc.counters().values()) and (got["sum_i"] > 0).all() and not got["sum_pol"].any()
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_a))


def test_a_scene_that_is_not_uploaded_is_refused(built, tmp_path):
    """WTGPU_ERR_INVALID (1) from the entry point itself, with the message; the Python method says the same before it gets there."""
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmPolar, FilmPolarSpec, load_library
    sc = stats_scene(tmp_path, 4)
    dev = torch.device("cuda", 0)
    films = (torch.zeros(37 * 23 * 4, dtype=torch.float64, device=dev), torch.zeros(37 * 23, dtype=torch.float64, device=dev),
             torch.zeros(37 * 23 * 4, dtype=torch.float64, device=dev))
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_polar_device(*films, 1)
    lib = load_library()
    spec, rec = FilmPolarSpec(), FilmPolar()
    rc = lib.wtgpu_film_polar_device(sc.handle, None, *(t.data_ptr() for t in films), 1, C.byref(spec), None, C.cast(C.pointer(rec), C.c_void_p), None, None)
    assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
