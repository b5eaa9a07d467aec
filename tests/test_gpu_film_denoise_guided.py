"""The feature-guided denoiser on the MI355X (wtgpu_film_denoise_guided_device; csrc/kernels_denoise.hip, the guided instantiations of k_denoise_filter)
against the host twin, bit for bit, film and residual, with and without the residual pointer: the same f32 arithmetic in one order on both sides
(wt/film_denoise.h), no tolerance.  The host twin itself is held to an f64 restatement by tests/test_film_denoise_guided.py, whose films and guides are
used here.  Covered at least once each, not as a cross product: P = 1, 3, 4, 12; ids alone, 1, 5 and 8 guide planes; with and without a mask; the
guides from global memory and staged in LDS (WTGPU_FILM_DENOISE_GUIDE_LDS), both directions in one launch and one launch each
(WTGPU_FILM_DENOISE_FUSED); 37 x 23 (three by two tiles, the last of each row and column partial) with (r, f) = (10, 3), (0, 2), (3, 0), 83 x 61
with (5, 2), and P = 3 at 83 x 61 with (10, 3), 8 planes and ids: the largest LDS request, where the staged form falls back to global memory."""
import ctypes as C
import json

import numpy as np
import pytest

from test_film_denoise import KW, PRIMES, SMALL, check_bad_pixels, denoise_films, films_with_bad_pixels, merged
from test_film_denoise_guided import GOLDEN, check_bad_guide, guide_planes, guide_with_bad_pixels, regions
from test_film_stats import F32, PLANES, SPE, checker, same_bits, stats_scene
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu
GUIDE_SETS = [(0, True), (1, False), (5, True), (8, False)]              # G, with ids


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_film_denoise_guided")
    return {(w, h, P): stats_scene(d, P, w, h).upload(0) for w, h in (SMALL, PRIMES) for P in PLANES}


def _device(sc, a, b, d_a=None, d_b=None, mask=None, guide=None, guide_scale=None, ids=None, residual=True, **kw):
    import torch
    d_a = _to_device(sc, a) if d_a is None else d_a
    d_b = _to_device(sc, b) if d_b is None else d_b
    d_mask, d_guide, d_ids = _to_device(sc, (mask, guide, None if ids is None else ids.view(np.int32)))
    got = sc.film_denoise_device(d_a, SPE, d_b, SPE, mask=d_mask, residual=residual, guide=d_guide, guide_scale=guide_scale, ids=d_ids, **KW, **kw)
    torch.cuda.synchronize(got["film"].device)
    return got["film"].cpu().numpy(), None if got["residual"] is None else got["residual"].cpu().numpy()


def _same(sc, a, b, label, d_a=None, d_b=None, **kw):
    """device = host twin: film and residual, and the film again without the residual pointer"""
    film, res = _device(sc, a, b, d_a, d_b, **kw)
    bare, none = _device(sc, a, b, d_a, d_b, residual=False, **kw)
    want = sc.film_denoise_host(a, SPE, b, SPE, residual=True, threads=16, **KW, **kw)
    assert same_bits(film, want["film"]), (label, "film", int((film.view(np.uint32) != want["film"].view(np.uint32)).sum()))
    assert same_bits(res, want["residual"]), (label, "residual")
    assert none is None and same_bits(bare, want["film"]), (label, "without the residual")
    return want["film"], want["residual"]


def _one_film(sc, size, P, r, f, seed, G, with_ids, masks=(None, True)):
    W, H = size
    a, b = denoise_films(H, W, P, seed)
    m, _ = merged(sc, a, b)
    guide, scale = guide_planes(H, W, G, seed + 1)
    ids = regions(H, W) if with_ids else None
    plain = sc.film_denoise_host(a, SPE, b, SPE, window=r, patch=f, **KW)["film"]
    for masked in masks:
        mask = checker(H, W) if masked else None
        film, _ = _same(sc, a, b, (size, P, r, f, G, with_ids, masked), mask=mask, guide=guide, guide_scale=scale, ids=ids, window=r, patch=f)
        assert r == 0 or (film != m).mean() > (0.5 if mask is None else 0.2)          # the filter had candidates to weigh ...
    assert r == 0 or not same_bits(film, plain)                                         # ... and the guides had their say


@pytest.mark.parametrize("r,f", [(10, 3), (0, 2), (3, 0)])
@pytest.mark.parametrize("P", sorted(PLANES))
def test_device_equals_host_twin(scenes, P, r, f):
    G, with_ids = GUIDE_SETS[(sorted(PLANES).index(P) + r) % 4]
    _one_film(scenes[SMALL + (P,)], SMALL, P, r, f, 100 + P, G, with_ids)


@pytest.mark.parametrize("P", sorted(PLANES))
def test_device_equals_host_twin_on_many_tiles(scenes, P):
    G, with_ids = GUIDE_SETS[(sorted(PLANES).index(P) + 2) % 4]
    _one_film(scenes[PRIMES + (P,)], PRIMES, P, 5, 2, 200 + P, G, with_ids)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_either_form_computes_the_same(built, tmp_path, monkeypatch, lds, fused):
    """The guides from global memory (0) or staged in LDS (1), one launch per direction (0) or both in one (1), each forced by its knob: the host
    twin's bits.  37 x 23, P = 1, (10, 3), 5 planes: 18,752 + 5 x 5,184 bytes, staged at the largest window.  83 x 61, P = 3, (7, 2), 5 planes and ids:
    the sizes of the benchmark, 31,524 + 3,600 + 18,000 bytes.  83 x 61, P = 3, (10, 3), 8 planes and ids: 46,976 + 5,184 + 41,472 bytes is beyond the
    64 KB of a launch, so the staged form reads these guides from global memory — the same bits either way."""
    monkeypatch.setenv("WTGPU_FILM_DENOISE_GUIDE_LDS", lds)
    monkeypatch.setenv("WTGPU_FILM_DENOISE_FUSED", fused)
    for size, P, r, f, G, with_ids, masks in ((SMALL, 1, 10, 3, 5, False, (None,)), (SMALL, 12, 3, 0, 8, True, (True,)), (PRIMES, 4, 5, 2, 1, True, (None,)),
                                              (PRIMES, 3, 7, 2, 5, True, (True,)), (PRIMES, 3, 10, 3, 8, True, (None,))):
        sc = stats_scene(tmp_path, P, *size).upload(0)
        _one_film(sc, size, P, r, f, 400 + P, G, with_ids, masks)
    W, H = SMALL
    sc = stats_scene(tmp_path, 12, W, H).upload(0)
    a, b = films_with_bad_pixels(H, W, 12, 11)
    guide, scale = guide_with_bad_pixels(H, W, 5, 12)
    _same(sc, a, b, ("non-finite film and guide pixels, forms", lds, fused), guide=guide, guide_scale=scale, ids=regions(H, W), window=3, patch=1)


def test_zero_scales_give_the_unguided_device_call(scenes):
    import torch
    for size, P, r, f in ((SMALL, 3, 10, 3), (PRIMES, 12, 5, 2), (SMALL, 4, 3, 1)):
        W, H = size
        sc = scenes[size + (P,)]
        a, b = denoise_films(H, W, P, 21)
        guide, _ = guide_planes(H, W, 5, 22)
        d_a, d_b = _to_device(sc, a), _to_device(sc, b)
        plain = sc.film_denoise_device(d_a, SPE, d_b, SPE, window=r, patch=f, residual=True, **KW)
        torch.cuda.synchronize(plain["film"].device)
        plain = plain["film"].cpu().numpy(), plain["residual"].cpu().numpy()
        for kw in (dict(guide=guide, guide_scale=0.0), dict(ids=np.full((H, W), 5, np.uint32)), dict(guide=guide[..., 0], guide_scale=0.0, ids=np.zeros((H, W), np.uint32))):
            got = _device(sc, a, b, d_a, d_b, window=r, patch=f, **kw)
            assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1]), (size, P, sorted(kw))


def test_the_same_memory_as_both_halves(scenes):
    W, H = SMALL
    for P, G, with_ids in ((3, 5, True), (4, 0, True)):
        sc = scenes[SMALL + (P,)]
        a, _ = denoise_films(H, W, P, 5)
        d_a = _to_device(sc, a)
        guide, scale = guide_planes(H, W, G, 6)
        _, res = _same(sc, a, a, ("A is B", P), d_a=d_a, d_b=d_a, guide=guide, guide_scale=scale, ids=regions(H, W) if with_ids else None, window=4, patch=1)
        assert not res.any()


def test_non_finite_film_and_guide_pixels(scenes):
    W, H = SMALL
    for P in (3, 12):
        sc = scenes[(W, H, P)]
        a, b = films_with_bad_pixels(H, W, P, 11)
        m, d = merged(sc, a, b)
        guide, scale = guide_planes(H, W, 5, 12)
        for r, f in ((3, 1), (6, 3)):
            film, res = _same(sc, a, b, ("non-finite film", P), guide=guide, guide_scale=scale, window=r, patch=f)
            check_bad_pixels(film.reshape(H, W, P), res.reshape(H, W, P), m.reshape(H, W, P), d.reshape(H, W, P), f)
        a, b = denoise_films(H, W, P, 11)
        bad, scale = guide_with_bad_pixels(H, W, 5, 12)
        _same(sc, a, b, ("non-finite guide", P), guide=bad, guide_scale=scale, ids=regions(H, W), window=6, patch=3)
        check_bad_guide(sc, a, b, bad, scale, _device, window=3, patch=1)


def test_a_mask_that_excludes_everything(scenes):
    for size in (SMALL, PRIMES):
        W, H = size
        sc = scenes[size + (12,)]
        a, b = denoise_films(H, W, 12, 6)
        mask = np.zeros((H, W), F32)
        mask[0, 0] = np.nan
        guide, scale = guide_planes(H, W, 5, 7)
        film, res = _same(sc, a, b, size, mask=mask, guide=guide, guide_scale=scale, ids=regions(H, W), window=5, patch=2)
        m, d = merged(sc, a, b)
        assert same_bits(film, m) and same_bits(res, d)


def test_rendered_half_films_with_first_hit_guides(built):
    """cornell_box polarimetric, 4 + 4 samples per element through render_to_noise(halves=True); the guide is first_hit_guides' — Scene.first_hit(samples=0)
    on the device, normals, log depth, coverage, the shape map — with its untuned default scales.  Device = host twin on that input, and
    render.denoise(guides=True) is that call.  For the record only, no assertion on their order (the defaults are untuned): rel_l2 of the merged, the
    unguided and the guided film against a longer render; tests/golden/denoise_guided_measured.json has what was seen."""
    import torch
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import denoise, first_hit_guides, render_to_noise
    sc = Scene("cornell_box", polarimetric=1, res=24, mesh_detail=0, crop_of=1440, lut=(64, 64)).upload(0)
    films, spp, _, (d_a, d_b) = render_to_noise(sc, 0.0, max_spp=8, chunk_spp=4, seed=3, halves=True)
    guide, scales, ids = first_hit_guides(sc)
    torch.cuda.synchronize(films[0].device)
    assert guide.shape == (sc.height, sc.width, 5) and guide.dtype == torch.float32 and guide.is_cuda and ids.dtype == torch.int32 and len(scales) == 5
    assert torch.isfinite(guide).all() and (guide[..., 4] > 0).any()
    a, b = (tuple(t.cpu().numpy() for t in half) for half in (d_a, d_b))
    h_guide, h_ids = guide.cpu().numpy(), ids.cpu().numpy().view(np.uint32)
    got = denoise(sc, d_a, d_b, 4, guides=(guide, scales, ids))
    auto = denoise(sc, d_a, d_b, 4, guides=True)
    want = denoise(sc, a, b, 4, guides=(h_guide, scales, h_ids))
    plain = denoise(sc, a, b, 4)
    for t in (got, auto):
        assert same_bits(t["film"].cpu().numpy(), want["film"]) and same_bits(t["residual"].cpu().numpy(), want["residual"])
    assert got["residual_rel"] == pytest.approx(want["residual_rel"], rel=1e-12) and want["residual_rel"] > 0 and np.isfinite(want["film"]).all()
    assert not same_bits(want["film"], plain["film"])
    long = render(sc, 256, seed=5)
    ref = sc.develop_device(*_to_device(sc, long), 256).cpu().numpy().reshape(want["film"].shape)[..., 0].astype(np.float64)
    m = sc.develop_device(*films, 8).cpu().numpy().reshape(want["film"].shape)[..., 0].astype(np.float64)
    rel = lambda t: float(np.sqrt(((t - ref) ** 2).sum() / (ref ** 2).sum()))
    seen = json.load(open(GOLDEN))["rendered_cornell_box"]
    print(f"film_denoise guided on cornell_box 24 x 24, 4 + 4 spe against 256 spe: rel_l2 merged {rel(m):.4f} unguided {rel(plain['film'][..., 0].astype(np.float64)):.4f} "
          f"guided {rel(want['film'][..., 0].astype(np.float64)):.4f} residual_rel {want['residual_rel']:.4f} (recorded: {seen['rel_l2_merged']} / "
          f"{seen['rel_l2_unguided']} / {seen['rel_l2_guided']})")


def test_guided_denoise_between_renders_changes_nothing(built):
    """As test_gpu_film_denoise.py's: the call counts nothing and leaves the films it reads alone."""
    import torch
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import first_hit_guides
    sc = Scene("furnace_path", polarimetric=1, res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_a, d_b = _to_device(sc, a), _to_device(sc, render(sc, 2, seed=7))
    guide, scales, ids = first_hit_guides(sc)
    sc.reset_counters()
    got = sc.film_denoise_device(d_a, 2, d_b, 2, residual=True, guide=guide, guide_scale=scales, ids=ids)
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
    from wave_tracer_amd.api import FilmDenoiseGuides, FilmDenoiseSpec, load_library
    sc = stats_scene(tmp_path, 4)
    dev = torch.device("cuda", 0)
    films = (torch.zeros(37 * 23 * 4, dtype=torch.float64, device=dev), torch.zeros(37 * 23, dtype=torch.float64, device=dev),
             torch.zeros(37 * 23 * 4, dtype=torch.float64, device=dev))
    guide, ids = torch.zeros((23, 37, 2), dtype=torch.float32, device=dev), torch.zeros((23, 37), dtype=torch.int32, device=dev)
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_denoise_device(films, 1, films, 1, guide=guide, ids=ids)
    lib = load_library()
    spec, guides = FilmDenoiseSpec(3, 1, 0, 0, 0.45, 1.0, 1e-10, 0.0), FilmDenoiseGuides(2, 1)
    out = torch.zeros(37 * 23 * 4, dtype=torch.float32, device=dev)
    rc = lib.wtgpu_film_denoise_guided_device(sc.handle, None, *(t.data_ptr() for t in films), 1, *(t.data_ptr() for t in films), 1, C.byref(spec), C.byref(guides),
                                              guide.data_ptr(), ids.data_ptr(), None, out.data_ptr(), None)
    assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
    # what the device method says itself: a guide that is not a tensor on the scene's device
    up = stats_scene(tmp_path, 4).upload(0)
    with pytest.raises(ValueError, match="guide: .* a tensor on cuda:0"):
        up.film_denoise_device(films, 1, films, 1, guide=np.zeros((23, 37, 2), F32))
    with pytest.raises(ValueError, match="ids: .* a tensor on cuda:0"):
        up.film_denoise_device(films, 1, films, 1, ids=ids.cpu())
