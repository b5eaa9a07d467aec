"""The denoiser of two half-films on the MI355X (wtgpu_film_denoise_device; csrc/kernels_denoise.hip) against the host twin, bit for bit, film and
residual: the same f32 arithmetic in one order on both sides (wt/film_denoise.h), no tolerance.  The host twin itself is held to an f64 numpy
restatement by tests/test_film_denoise.py, whose films are used here: P = 1, 3, 4 and 12 planes at 37 x 23 (three by two 16 x 16 tiles, the last of
each row and column partial) with the largest window and patch, without a window, without a patch; at 83 x 61 (six by four tiles: interior, edge
and partial ones); the largest halo at 83 x 61; each with and without a mask, and in either form of the filter kernel forced by WTGPU_FILM_DENOISE_FUSED.  Then the same
memory as both halves, non-finite pixels, a mask that excludes everything, rendered half-films, and what the call leaves alone."""
import ctypes as C

import numpy as np
import pytest

from test_film_denoise import KW, PRIMES, SMALL, check_bad_pixels, denoise_films, films_with_bad_pixels, merged
from test_film_stats import F32, PLANES, SPE, checker, same_bits, stats_scene
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_film_denoise")
    return {(w, h, P): stats_scene(d, P, w, h).upload(0) for w, h in (SMALL, PRIMES) for P in PLANES}


def _same(sc, a, b, mask, label, d_a=None, d_b=None, **kw):
    import torch
    d_a = _to_device(sc, a) if d_a is None else d_a
    d_b = _to_device(sc, b) if d_b is None else d_b
    d_mask, = _to_device(sc, (mask,))
    got = sc.film_denoise_device(d_a, SPE, d_b, SPE, mask=d_mask, residual=True, **KW, **kw)
    bare = sc.film_denoise_device(d_a, SPE, d_b, SPE, mask=d_mask, **KW, **kw)
    torch.cuda.synchronize(got["film"].device)
    want = sc.film_denoise_host(a, SPE, b, SPE, mask=mask, residual=True, threads=16, **KW, **kw)
    film, res = got["film"].cpu().numpy(), got["residual"].cpu().numpy()
    assert same_bits(film, want["film"]), (label, kw, "film", int((film.view(np.uint32) != want["film"].view(np.uint32)).sum()))
    assert same_bits(res, want["residual"]), (label, kw, "residual")
    assert bare["residual"] is None and same_bits(bare["film"].cpu().numpy(), want["film"]), (label, kw, "without the residual")
    return want


def _one_film(sc, size, P, r, f, seed):
    W, H = size
    a, b = denoise_films(H, W, P, seed)
    m, _ = merged(sc, a, b)
    for mask in (None, checker(H, W)):
        want = _same(sc, a, b, mask, (size, P, mask is not None), window=r, patch=f)
        assert r == 0 or (want["film"] != m).mean() > (0.5 if mask is None else 0.2)          # the filter had candidates to weigh


@pytest.mark.parametrize("r,f", [(10, 3), (0, 2), (3, 0)])
@pytest.mark.parametrize("P", sorted(PLANES))
def test_device_equals_host_twin(scenes, P, r, f):
    _one_film(scenes[SMALL + (P,)], SMALL, P, r, f, 100 + P)


@pytest.mark.parametrize("P", sorted(PLANES))
def test_device_equals_host_twin_on_many_tiles(scenes, P):
    _one_film(scenes[PRIMES + (P,)], PRIMES, P, 5, 2, 200 + P)


def test_device_equals_host_twin_with_the_largest_halo(scenes):
    _one_film(scenes[PRIMES + (3,)], PRIMES, 3, 10, 3, 303)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_either_form_computes_the_same(built, tmp_path, monkeypatch, fused):
    """The two forms the A/B of csrc/kernels_denoise.hip chooses between by the film's planes — one launch per direction, the first direction's
    result through scratch memory (0), and both directions in one launch (1) — each forced by the knob for every plane count: the host twin's bits."""
    monkeypatch.setenv("WTGPU_FILM_DENOISE_FUSED", fused)
    for size, P, r, f in ((SMALL, 1, 10, 3), (SMALL, 12, 3, 0), (PRIMES, 4, 5, 2), (PRIMES, 3, 5, 2)):
        sc = stats_scene(tmp_path, P, *size).upload(0)
        _one_film(sc, size, P, r, f, 400 + P)
    a, b = films_with_bad_pixels(SMALL[1], SMALL[0], 12, 11)
    _same(stats_scene(tmp_path, 12, *SMALL).upload(0), a, b, None, ("non-finite pixels, form", fused), window=3, patch=1)


def test_the_same_memory_as_both_halves(scenes):
    for P in (3, 4):
        sc = scenes[SMALL + (P,)]
        a, _ = denoise_films(SMALL[1], SMALL[0], P, 5)
        d_a = _to_device(sc, a)
        want = _same(sc, a, a, None, ("A is B", P), d_a=d_a, d_b=d_a, window=4, patch=1)
        assert not want["residual"].any()


def test_non_finite_pixels(scenes):
    W, H = SMALL
    for P in (3, 12):
        sc = scenes[(W, H, P)]
        a, b = films_with_bad_pixels(H, W, P, 11)
        m, d = merged(sc, a, b)
        for r, f in ((3, 1), (6, 3)):
            want = _same(sc, a, b, None, ("non-finite", P), window=r, patch=f)
            check_bad_pixels(want["film"].reshape(H, W, P), want["residual"].reshape(H, W, P), m.reshape(H, W, P), d.reshape(H, W, P), f)


def test_a_mask_that_excludes_everything(scenes):
    for size in (SMALL, PRIMES):
        sc = scenes[size + (12,)]
        a, b = denoise_films(size[1], size[0], 12, 6)
        mask = np.zeros((size[1], size[0]), F32)
        mask[0, 0] = np.nan
        want = _same(sc, a, b, mask, size, window=5, patch=2)
        m, d = merged(sc, a, b)
        assert same_bits(want["film"], m) and same_bits(want["residual"], d)


def test_rendered_half_films(built):
    """cornell_box polarimetric, 4 + 4 samples per element through render_to_noise(halves=True): device = host twin on the downloaded halves, and
    render.denoise gives the same from the torch films as from the numpy ones.  For the record only (no assertion: eight samples per element are
    eight samples per element): rel_l2 of the merged and of the denoised film against a longer render."""
    import torch
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import denoise, render_to_noise
    sc = Scene("cornell_box", polarimetric=1, res=24, mesh_detail=0, crop_of=1440, lut=(64, 64)).upload(0)
    films, spp, _, (d_a, d_b) = render_to_noise(sc, 0.0, max_spp=8, chunk_spp=4, seed=3, halves=True)
    torch.cuda.synchronize(films[0].device)
    assert spp == 8 and all(torch.equal(x + y, t) for t, x, y in zip(films, d_a, d_b))
    a, b = (tuple(t.cpu().numpy() for t in half) for half in (d_a, d_b))
    got, want = denoise(sc, d_a, d_b, 4), denoise(sc, a, b, 4)
    assert same_bits(got["film"].cpu().numpy(), want["film"]) and same_bits(got["residual"].cpu().numpy(), want["residual"])
    assert got["residual_rel"] == pytest.approx(want["residual_rel"], rel=1e-12) and want["residual_rel"] > 0 and np.isfinite(want["film"]).all()
    long = render(sc, 256, seed=5)
    ref = sc.develop_device(*_to_device(sc, long), 256).cpu().numpy().reshape(want["film"].shape)[..., 0].astype(np.float64)
    m = sc.develop_device(*films, 8).cpu().numpy().reshape(want["film"].shape)[..., 0].astype(np.float64)
    rel = lambda t: float(np.sqrt(((t - ref) ** 2).sum() / (ref ** 2).sum()))
    print(f"film_denoise on cornell_box 24 x 24, 4 + 4 spe against 256 spe: rel_l2 merged {rel(m):.4f} denoised {rel(want['film'][..., 0].astype(np.float64)):.4f} "
          f"residual_rel {want['residual_rel']:.4f}")


def test_denoise_between_renders_changes_nothing(built):
    """As test_gpu_film_compare.py::test_compare_between_renders_changes_nothing: the call counts nothing and leaves the films it reads alone."""
    import torch
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", polarimetric=1, res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_a, d_b = _to_device(sc, a), _to_device(sc, render(sc, 2, seed=7))
    sc.reset_counters()
    got = sc.film_denoise_device(d_a, 2, d_b, 2, residual=True)
    torch.cuda.synchronize(got["film"].device)
    assert all(v == 0 for v in sc.counters().values()) and got["film"].any() and torch.isfinite(got["film"]).all()
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_a))


def test_a_scene_that_is_not_uploaded_is_refused(built, tmp_path):
    """WTGPU_ERR_INVALID (1) from the entry point itself, with the message; the Python method says the same before it gets there."""
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmDenoiseSpec, load_library
    sc = stats_scene(tmp_path, 4)
    dev = torch.device("cuda", 0)
    films = (torch.zeros(37 * 23 * 4, dtype=torch.float64, device=dev), torch.zeros(37 * 23, dtype=torch.float64, device=dev),
             torch.zeros(37 * 23 * 4, dtype=torch.float64, device=dev))
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_denoise_device(films, 1, films, 1)
    lib = load_library()
    spec = FilmDenoiseSpec(3, 1, 0, 0, 0.45, 1.0, 1e-10, 0.0)
    out = torch.zeros(37 * 23 * 4, dtype=torch.float32, device=dev)
    rc = lib.wtgpu_film_denoise_device(sc.handle, None, *(t.data_ptr() for t in films), 1, *(t.data_ptr() for t in films), 1, C.byref(spec), None, out.data_ptr(), None)
    assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
