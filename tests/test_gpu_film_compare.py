"""Film comparison on the MI355X (wtgpu_film_compare_device; csrc/kernels_compare.hip) against the host twin, bit for bit: the four counts,
max_abs and argmax, the five sums and the difference plane — the additions have one order and the maximum's order is total
(wt/film_compare.h), so there is nothing to tolerate.  The host twin itself is held to a numpy restatement by tests/test_film_compare.py, whose
pairs and options are used here: P = 1, 3, 4, 12 planes at 37 x 23 (851 pixels: a part of one block, chunks that end inside the film) and one
pair at 256 x 192 (192 chunks: 48 blocks, a second level of chunk sums); P = 3 and 12 at 257 x 256 (257 chunks, then 2, then 1: the reduction's
loop runs twice).  Then rendered films, render_to_noise against the one-shot render, and
what the calls leave alone."""
import ctypes as C

import numpy as np
import pytest

from test_film_compare import EARLY, FIELDS, LATE, NO_PIXEL, SPE_A, SPE_B, films_of, late_tie_films, pairs
from test_film_stats import F32, LEVELS, PLANES, checker, device_scenes, option_cases, same_bits, stats_scene
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (256, 192)]
DERIVED = ("rmse", "mean_abs", "rel_l2", "rel_mse")


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_film_compare")
    return device_scenes(d, SIZES)


def _same(sc, fa, d_fa, spe_a, fb, d_fb, spe_b, mask, d_mask, label, **kw):
    got = sc.film_compare_device(d_fa, spe_a, d_fb, spe_b, mask=d_mask, diff=True, **kw)
    want = sc.film_compare_host(fa, spe_a, fb, spe_b, mask=mask, diff=True, threads=16, **kw)
    for k in FIELDS + DERIVED:
        assert same_bits(got[k], want[k]), (label, kw, k, got[k], want[k])
    assert same_bits(got["diff"].cpu().numpy(), want["diff"]), (label, kw, "diff")
    return got


@pytest.mark.parametrize("P", sorted(PLANES))
def test_device_equals_host_twin(scenes, P):
    W, H = SIZES[0]
    sc = scenes[(W, H, P)]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    d_mask, = _to_device(sc, (mask,))
    for label, fa, fb in pairs(P):
        d_fa, d_fb = _to_device(sc, fa), _to_device(sc, fb)
        spe_b = SPE_B if label == "two draws" else SPE_A
        for s, abs_, lum, masked in option_cases(channels, stokes):
            got = _same(sc, fa, d_fa, SPE_A, fb, d_fb, spe_b, mask if masked else None, d_mask if masked else None, (P, label), stokes_component=s, abs=abs_,
                        luminance=lum, eps=1e-4 if s % 2 == 0 else 3e-9)
            assert got["n"][0] == (int((mask > 0).sum()) if masked else W * H) and got["diff"].shape == (H, W, channels + lum)
            if label == "two draws":
                assert got["n_differ"].all() and got["n_nonfinite"].all() and (got["argmax"] < W * H).all()
            if label == "itself":
                assert not got["n_differ"].any() and (got["argmax"] == NO_PIXEL).all()


@pytest.mark.parametrize("P", sorted(PLANES))
def test_device_equals_host_twin_on_many_chunks(scenes, P):
    _many_chunks(scenes, SIZES[1], P)


@pytest.mark.parametrize("P", [3, 12])
def test_device_equals_host_twin_over_two_levels(scenes, P):
    """257 x 256: k_film_finish goes round its loop twice, the second time over what the first wrote."""
    _many_chunks(scenes, LEVELS, P)


def test_a_late_maximum_and_a_tie_across_the_wavefronts_records(scenes):
    """257 x 256: 257 chunks on 65 blocks, 260 wavefront records — k_film_finish's 256 threads go round the records twice.  The maximum is in the
    last chunk (record 256, the second round) with its equal in chunk 3 (record 3): argmax is the smaller pixel; without the early one, the late."""
    sc = scenes[LEVELS + (3,)]
    for early in (True, False):
        fa, fb = late_tie_films(early)
        got = _same(sc, fa, _to_device(sc, fa), SPE_A, fb, _to_device(sc, fb), SPE_A, None, None, ("late tie", early))
        assert got["argmax"].tolist() == [(EARLY if early else LATE) + c for c in range(3)] and got["max_abs"].tolist() == [2.0] * 3


def _many_chunks(scenes, size, P):
    W, H = size
    sc = scenes[(W, H, P)]
    _, _, channels, stokes = PLANES[P]
    fa, fb = films_of(P, 500 + P, H, W), films_of(P, 600 + P, H, W)
    d_fa, d_fb = _to_device(sc, fa), _to_device(sc, fb)
    mask = checker(H, W)
    d_mask, = _to_device(sc, (mask,))
    for s, abs_, lum, masked in option_cases(channels, stokes):
        got = _same(sc, fa, d_fa, SPE_A, fb, d_fb, SPE_B, mask if masked else None, d_mask if masked else None, (P, size), stokes_component=s, abs=abs_,
                    luminance=lum)
        assert got["n"][0] == (int((mask > 0).sum()) if masked else W * H) and got["n_differ"].all()


def test_the_same_pointers_twice(scenes):
    """A == B: the kernel reads the same memory through both sets of pointers."""
    for W, H in SIZES:
        sc = scenes[(W, H, 12)]
        fa = films_of(12, 31, H, W)
        d_fa = _to_device(sc, fa)
        got = _same(sc, fa, d_fa, SPE_A, fa, d_fa, SPE_A, None, None, (W, H, "A == B"), stokes_component=2, luminance=True)
        assert got["n_nonfinite"].all() and not got["n_nonfinite_mismatch"].any() and not got["n_differ"].any() and not got["sum_sq"].any()
        assert (got["argmax"] == NO_PIXEL).all() and same_bits(got["sum_a_sq"], got["sum_b_sq"])


def test_a_mask_that_excludes_everything(scenes):
    for W, H in SIZES:
        sc = scenes[(W, H, 3)]
        fa, fb = films_of(3, 5, H, W), films_of(3, 6, H, W)
        mask = np.zeros((H, W), F32)
        mask[0, 0] = np.nan
        got = _same(sc, fa, _to_device(sc, fa), SPE_A, fb, _to_device(sc, fb), SPE_B, mask, _to_device(sc, (mask,))[0], (W, H), luminance=True)
        assert not got["n"].any() and not got["sum_a_sq"].any() and (got["argmax"] == NO_PIXEL).all() and not got["diff"].any()


def test_rendered_films(built):
    """Two renders of double_slits with different seeds: device = host twin on the downloaded films, and noise_estimate gives the same float from
    the torch films as from the numpy ones."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films, noise_estimate
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    sc = Scene("double_slits", res=96, lut=(128, 128)).upload(0)
    d_a, d_b = alloc_films(sc, dev), alloc_films(sc, dev)
    sc.render_into(*d_a, 0, 4, 17, st)
    sc.render_into(*d_b, 0, 4, 18, st)
    torch.cuda.synchronize(dev)
    a, b = (tuple(t.cpu().numpy() for t in f) for f in (d_a, d_b))
    got = _same(sc, a, d_a, 4, b, d_b, 4, None, None, "double_slits")
    assert got["n_differ"][0] > 0 and got["n_nonfinite"][0] == 0 and 0 < got["rel_l2"][0] < 10
    est = noise_estimate(sc, d_a, d_b, 4)
    assert est == noise_estimate(sc, a, b, 4) and 0 < est < 1


def test_render_to_noise_equals_the_one_shot_render(built):
    """furnace_path, four samples as 1 + 1 + 1 + 1 into alternating halves, then A += B: the film of render(sc, 4) but for the order of the f64
    additions the atomics make (as two renders of the same samples differ: test_gpu_film_stats.py::test_stats_between_renders_change_nothing),
    judged by the new call itself; and the counters of the one-shot render."""
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import render_to_noise
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    one = render(sc, 4, seed=6)
    c_one = sc.counters()
    sc.reset_counters()
    films, spp, history = render_to_noise(sc, 0.0, max_spp=4, chunk_spp=1, seed=6)
    assert sc.counters() == c_one and c_one["samples"] > 0
    assert spp == 4 and [s for s, _ in history] == [2, 4] and all(e > 0 for _, e in history)
    d_one = _to_device(sc, one)
    got = sc.film_compare_device(films, 4, d_one, 4, luminance=sc.spectral_channels == 3)
    print(f"render_to_noise against the one-shot render: rel_l2 {got['rel_l2']}, max_abs {got['max_abs']}, n_differ {got['n_differ']}")
    assert (got["rel_l2"] <= 1e-12).all() and not got["n_nonfinite"].any()
    for x, t in zip(one, films):
        y = t.cpu().numpy()
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)


def test_compare_between_renders_changes_nothing(built):
    """As test_gpu_film_stats.py::test_stats_between_renders_change_nothing: the call counts nothing and leaves the films it reads alone."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_a, d_b = _to_device(sc, a), _to_device(sc, (2 * a[0], a[1], a[2]))
    got = sc.film_compare_device(d_a, 2, d_b, 2, luminance=True, diff=True)
    assert all(v == 0 for v in sc.counters().values()) and got["n_differ"].any()
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_a)) and same_bits(2 * a[0], d_b[0].cpu().numpy())


def test_a_scene_that_is_not_uploaded_is_refused(built, tmp_path):
    """WTGPU_ERR_INVALID (1) from the entry point itself, with the message; the Python method says the same before it gets there."""
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmCompare, FilmCompareSpec, load_library
    sc = stats_scene(tmp_path, 1)
    dev = torch.device("cuda", 0)
    films = tuple(torch.zeros(37 * 23, dtype=torch.float64, device=dev) for _ in range(3))
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_compare_device(films, 1, films, 1)
    lib = load_library()
    spec, rec = FilmCompareSpec(0, 0, 1e-4), FilmCompare()
    p = [t.data_ptr() for t in films]
    rc = lib.wtgpu_film_compare_device(sc.handle, None, *p, 1, *p, 1, C.byref(spec), None, C.cast(C.pointer(rec), C.c_void_p), None)
    assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
