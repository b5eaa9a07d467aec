"""Film statistics on the MI355X (wtgpu_film_stats_device; csrc/kernels_stats.hip) against the host twin, bit for bit: every counter, every bin,
min / max / min_positive and the sum — the classification compares f32 values with one f32 edge table and the additions have one order
(wt/film_stats.h), so there is nothing to tolerate.  The host twin itself is held to a numpy restatement by tests/test_film_stats.py, whose
films and options are used here: P = 1, 3, 4, 12 planes at 37 x 23 (851 pixels: a part of one block, chunks that end inside the film) and at
256 x 192 (192 chunks: 48 blocks, a second level of chunk sums); P = 3 and 12 at 257 x 256 (257 chunks, then 2, then 1: the reduction's loop
runs twice)."""
import numpy as np
import pytest

from test_film_stats import BINS, F32, LEVELS, PLANES, RANGES, SPE, checker, device_scenes, option_cases, restate_edges, same_bits, stats_films, stats_scene
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (256, 192)]
FIELDS = ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above", "min", "max", "min_positive", "sum", "hist", "edges")


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_film_stats")
    return device_scenes(d, SIZES)


def _same(sc, films, d_films, mask, d_mask, label, spe=SPE, **kw):
    got = sc.film_stats_device(*d_films, spe, mask=d_mask, **kw)
    want = sc.film_stats_host(*films, spe, mask=mask, threads=16, **kw)
    for k in FIELDS:
        assert same_bits(got[k], want[k]), (label, kw, k, got[k], want[k])
    assert got["range"] == want["range"] and got["bins"] == want["bins"]
    return got


@pytest.mark.parametrize("P", sorted(PLANES))
@pytest.mark.parametrize("size", SIZES)
def test_device_equals_host_twin(scenes, size, P):
    W, H = size
    sc = scenes[(W, H, P)]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    d_mask, = _to_device(sc, (mask,))
    for bins in BINS:
        for k, (scale, (lo, hi)) in enumerate(RANGES.items()):
            films = stats_films(H, W, channels, stokes, 200 + P + bins, restate_edges(scale, lo, hi, bins), infinities=bool((bins + k) % 2))
            d_films = _to_device(sc, films)
            for s, abs_, lum, masked in option_cases(channels, stokes):
                got = _same(sc, films, d_films, mask if masked else None, d_mask if masked else None, (W, H, P), stokes_component=s, scale=scale, range=(lo, hi), bins=bins,
                            abs=abs_, luminance=lum)
                assert got["n"][0] == (int((mask > 0).sum()) if masked else W * H) and got["hist"].shape == (channels + lum, bins)
                assert bins == 0 or got["hist"].any()


@pytest.mark.parametrize("P", [3, 12])
def test_device_equals_host_twin_over_two_levels(scenes, P):
    """257 x 256: k_film_stats_finish goes round its loop twice, the second time over what the first wrote; 256 bins, every option case."""
    W, H = LEVELS
    sc = scenes[(W, H, P)]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    d_mask, = _to_device(sc, (mask,))
    lo, hi = RANGES["dB"]
    films = stats_films(H, W, channels, stokes, 700 + P, restate_edges("dB", lo, hi, 256))
    d_films = _to_device(sc, films)
    for s, abs_, lum, masked in option_cases(channels, stokes):
        got = _same(sc, films, d_films, mask if masked else None, d_mask if masked else None, (W, H, P), stokes_component=s, range=(lo, hi), bins=256, abs=abs_,
                    luminance=lum)
        assert got["n"][0] == (int((mask > 0).sum()) if masked else W * H) and got["hist"].shape == (channels + lum, 256) and got["hist"].any()


def test_all_values_in_one_of_4096_bins(scenes):
    """Every block counts all its elements into ONE LDS word and flushes one bin: 49152 elements in bin 1234, per plane."""
    W, H = 256, 192
    sc = scenes[(W, H, 12)]
    edges = restate_edges("dB", -50, 10, 4096)
    x = float(np.nextafter(edges[1234], F32(np.inf)))
    films = (np.full((H, W, 12), x), np.ones((H, W)), np.zeros((H, W, 12)))
    got = _same(sc, films, _to_device(sc, films), None, None, "one bin", stokes_component=2, range=(-50, 10), bins=4096, luminance=True)
    assert got["hist"][:3, 1234].tolist() == [W * H] * 3 and got["hist"][:3].sum() == 3 * W * H and got["hist"][3].sum() == W * H
    assert (got["min"][:3] == F32(x)).all() and (got["max"][:3] == F32(x)).all() and (got["sum"][:3] == W * H * float(F32(x))).all()


def test_a_mask_that_excludes_everything(scenes):
    for W, H in SIZES:
        sc = scenes[(W, H, 3)]
        films = stats_films(H, W, 3, 1, 5, restate_edges("dB", -50, 10, 7))
        mask = np.zeros((H, W), F32)
        mask[0, 0] = np.nan
        got = _same(sc, films, _to_device(sc, films), mask, _to_device(sc, (mask,))[0], (W, H), range=(-50, 10), bins=7, luminance=True)
        assert not got["n"].any() and not got["hist"].any() and (got["sum"] == 0).all()
        assert np.isnan(got["min"]).all() and np.isnan(got["max"]).all() and np.isnan(got["min_positive"]).all()


def test_rendered_films(built):
    """A rendered double_slits film (virtual-plane sensor, monochromatic), with and without a range of its own; and the perspective view of the
    same scene (RGB) under the by-geometry mask computed on the device: device = host twin, and the masked count is the mask's."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films, auto_db_range
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    sc = Scene("double_slits", res=96, lut=(128, 128)).upload(0)
    d_films = alloc_films(sc, dev)
    sc.render_into(*d_films, 0, 4, 17, st)
    torch.cuda.synchronize(dev)
    films = tuple(t.cpu().numpy() for t in d_films)
    a = _same(sc, films, d_films, None, None, "double_slits", spe=4, range=(-18.0, 25.0), bins=256)          # double_slits.xml's dB range
    b = _same(sc, films, d_films, None, None, "double_slits, range=None", spe=4)
    assert a["hist"].any() and b["hist"].sum() == (sc.width * sc.height - b["n_zero"][0] - b["n_negative"][0] - b["n_nan"][0])
    assert auto_db_range(sc, d_films, 4) == auto_db_range(sc, films, 4)
    ov = Scene("double_slits_overview", res=32, lut=(64, 64)).upload(0)
    assert ov.info.sensor_type == 0 and ov.spectral_channels == 3
    d_mask = ov.sensor_mask(shapes=np.arange(ov.info.n_shapes) % 2, seed=3)
    d_films = alloc_films(ov, dev)
    ov.render_into(*d_films, 0, 4, 18, st)
    torch.cuda.synchronize(dev)
    films, mask = tuple(t.cpu().numpy() for t in d_films), d_mask.cpu().numpy()
    c = _same(ov, films, d_films, mask, d_mask, "overview", spe=4, scale="linear", range=(1e-4, 2.0), bins=64, luminance=True)
    assert c["n"].tolist() == [int((mask > 0).sum())] * 4


def test_stats_between_renders_change_nothing(built):
    """As test_gpu_develop.py::test_develop_between_renders_changes_nothing: the calls count nothing and leave the films they read alone."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_films = _to_device(sc, a)
    got = sc.film_stats_device(*d_films, 2, luminance=True)
    assert all(v == 0 for v in sc.counters().values()) and got["hist"].any()
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_films))


def test_a_scene_that_is_not_uploaded_is_refused(built, tmp_path):
    """WTGPU_ERR_INVALID (1) from the entry point itself, with the message; the Python method says the same before it gets there."""
    import ctypes as C
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmStats, FilmStatsSpec, load_library
    sc = stats_scene(tmp_path, 1)
    dev = torch.device("cuda", 0)
    v, w, l = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (37 * 23, 37 * 23, 37 * 23))
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_stats_device(v, w, l, 1, range=(-50, 10))
    lib = load_library()
    spec, rec = FilmStatsSpec(0, 1, 0, 0, -50.0, 10.0), FilmStats()
    rc = lib.wtgpu_film_stats_device(sc.handle, None, v.data_ptr(), w.data_ptr(), l.data_ptr(), 1, C.byref(spec), None, C.cast(C.pointer(rec), C.c_void_p), None)
    assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
