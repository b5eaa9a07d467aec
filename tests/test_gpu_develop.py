"""Film development and tonemapping on the MI355X (wtgpu_develop_device, wtgpu_tonemap_device; csrc/kernels_develop.hip): k_develop against
wtgpu_develop bit for bit, k_develop_tonemap against its host twin bit for bit where no libm function is called and against the f64
restatement of tests/test_tonemap.py otherwise (tolerance: 10 x the difference measured on the MI355X, tests/golden/tonemap_measured.json
"device/..."; the derivation and the 1e-5 alarm are test_tonemap.py's).  Synthetic films on scenes chosen for their plane counts P = 1, 3, 4, 12,
at 37 x 23 (851 pixels: no multiple of a wavefront or a block, odd P on odd sizes) and 256 x 192; one rendered film; and development between
two renders changes nothing."""
import numpy as np
import pytest

from test_sensor_mask import _write
from test_tonemap import (F32, FILM_CASES, LIBM_OPS, MODES, MONO, RGB, check_measured, film_xml, grey_table, make_films, nan_equal_maxdiff, quantise,
                          random_table, restate, same_bits)

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (256, 192)]
PLANES = [(MONO, False, 1, 1), (RGB, False, 3, 1), (RGB, True, 3, 4), (MONO, True, 1, 4)]     # response, polarimetric, channels, stokes


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    """{(width, height, P): (uploaded scene, channels, stokes)}"""
    from wave_tracer_amd import Scene
    d = tmp_path_factory.mktemp("develop")
    out = {}
    for W, H in SIZES:
        for resp, pol, channels, stokes in PLANES:
            sc = Scene.from_xml(_write(d, f"f{W}_{channels}_{stokes}.xml", film_xml(response=resp, width=W, height=H, polarimetric=pol))).upload(0)
            assert (sc.width, sc.height, sc.spectral_channels, sc.stokes) == (W, H, channels, stokes)
            out[(W, H, channels * stokes)] = (sc, channels, stokes)
    return out


def _to_device(sc, films):
    import torch
    dev = torch.device("cuda", sc.device)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in films)


def _host(t):
    import torch
    torch.cuda.synchronize(t.device)
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def test_develop_device_equals_wtgpu_develop(scenes):
    """IEEE f64 divide, multiply, add and one conversion, contraction off on both sides: bit for bit, for P = 1, 3, 4, 12, spe 0 and 7, the
    zero-weight pixels, the light-only and the no-light film."""
    from wave_tracer_amd import develop
    for (W, H, P), (sc, channels, stokes) in scenes.items():
        for kind, spe in FILM_CASES + [("random", 0)]:
            films = make_films(H, W, channels, stokes, 21, kind)
            got = _host(sc.develop_device(*_to_device(sc, films), spe))
            want = develop(sc, *films, spe)
            assert got.shape == (H, W, P) and got.dtype == F32 and same_bits(got, want), (W, H, P, kind, spe, int((got != want).sum()))


def test_tonemap_device_equals_host_where_no_libm_is_called(scenes):
    """linear, the three modes, grey / random tables, every Stokes component, f32 / u8 / u16, with and without the mask: bit for bit the host twin."""
    for (W, H, P), (sc, channels, stokes) in scenes.items():
        mask = np.random.default_rng(3).uniform(-0.2, 1.2, (H, W)).astype(F32)
        mask.reshape(-1)[:3] = [np.nan, 0.0, 1.0]
        d_mask = _to_device(sc, (mask,))[0]
        for kind, spe in (("edges", 0), ("random", 7)):
            films = make_films(H, W, channels, stokes, 11, kind)
            d_films = _to_device(sc, films)
            for k, mode in enumerate(MODES):
                tm = {"op": "linear", "mode": mode, "table": (grey_table(), random_table(5), random_table(1024))[(k + P) % 3]}
                for s in range(stokes):
                    for fmt in ("f32", "u8", "u16"):
                        for m, dm in ((None, None), (mask, d_mask)):
                            got = _host(sc.tonemap_device(*d_films, spe, tm, s, mask=dm, fmt=fmt))
                            want = sc.tonemap_host(*films, spe, tm, s, mask=m, fmt=fmt, threads=16)
                            assert same_bits(got, want), (W, H, P, kind, mode, s, fmt, m is not None, int((got != want).any(axis=-1).sum()))


def test_tonemap_device_gamma_srgb_db_against_the_f64_restatement(scenes):
    """f32 within 10 x the difference measured on the MI355X (below 1e-5); u8 / u16 within one code of the quantised restatement, every pixel;
    NaN where the restatement is NaN (code 0 in the integer formats)."""
    from wave_tracer_amd import imageio
    tables = [grey_table(), imageio.colour_table("turbo")]     # (why not a random table: test_tonemap.py, libm_cases)
    worst = {}
    for (W, H, P), (sc, channels, stokes) in scenes.items():
        for kind, spe in (("edges", 0), ("random", 7)):
            films = make_films(H, W, channels, stokes, 13, kind)
            d_films = _to_device(sc, films)
            for op in LIBM_OPS:
                for k, mode in enumerate(MODES):
                    tm, s = dict(op, mode=mode, table=tables[(k + stokes) % 2]), stokes - 1
                    want = restate(channels, stokes, *films, spe, tm, s)
                    got = _host(sc.tonemap_device(*d_films, spe, tm, s))
                    worst[op["op"]] = max(worst.get(op["op"], 0.0), nan_equal_maxdiff(got, want))
                    for fmt in ("u8", "u16"):
                        q = _host(sc.tonemap_device(*d_films, spe, tm, s, fmt=fmt)).astype(np.int64)
                        assert np.abs(q - quantise(want, fmt)).max() <= 1, (W, H, P, op, mode, fmt)
                        assert not q[np.isnan(want)].any()
    for op, m in sorted(worst.items()):
        check_measured(f"device/{op}", m)


def test_a_rendered_film(built):
    """double_slits at res 96, a few samples per element: the dB spec of scenes/diffraction_simple/double_slits.xml (the bundled scene has no file
    to take it from) with the grey table, against the restatement on the downloaded films; the picture is not empty.  Without a spec the
    bundled scene's default asks for a map the library does not tabulate."""
    import torch
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.render import alloc_films
    sc = Scene("double_slits", res=96, lut=(128, 128)).upload(0)
    dev = torch.device("cuda", 0)
    films = alloc_films(sc, dev)
    sc.render_into(*films, 0, 4, 17, torch.cuda.current_stream(dev).cuda_stream)
    tm = {"op": "dB", "mode": "select", "db_range": (-18.0, 25.0), "table": grey_table()}     # double_slits.xml:11-12,67-69
    got = _host(sc.tonemap_device(*films, 4, tm))
    v, w, l = (t.cpu().numpy() for t in films)
    want = restate(1, 1, v, w, l.reshape(v.shape), 4, tm)
    check_measured("device/rendered_double_slits_dB", nan_equal_maxdiff(got, want))
    assert ((got > 0) & (got < 1)).any() and got.shape == (sc.height, sc.width, 3)
    with pytest.raises(WtgpuError, match='"Magma".*pass a table'):
        sc.tonemap_device(*films, 4)


def test_develop_between_renders_changes_nothing(built):
    """As test_gpu_sensor_mask.py::test_mask_between_renders_changes_nothing: a develop_device and a tonemap_device between two renders of the
    same samples leave the counters identical and count nothing themselves."""
    import torch
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import alloc_films
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_films = _to_device(sc, a)
    dev_img = _host(sc.develop_device(*d_films, 2))
    pic = _host(sc.tonemap_device(*d_films, 2, fmt="u8"))       # the scene's own spec: sRGB / normal, no map needed
    assert all(v == 0 for v in sc.counters().values()) and dev_img.any() and pic.any()
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, _host(t)) for x, t in zip(a, d_films))     # the films the calls read are untouched


def test_render_develop_device_equals_render_develop(built):
    """What render_with_preview now shows: render.develop_device on the device films = render.develop on the downloaded ones, bit for bit."""
    import torch
    from wave_tracer_amd import Scene, develop
    from wave_tracer_amd.render import alloc_films, develop_device
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    dev = torch.device("cuda", 0)
    films = alloc_films(sc, dev)
    sc.render_into(*films, 0, 2, 9, torch.cuda.current_stream(dev).cuda_stream)
    got = develop_device(sc, *films, 2)
    torch.cuda.synchronize(dev)
    want = develop(sc, *(t.cpu().numpy() for t in films), 2)
    assert got.dtype == F32 and got.shape == want.shape and same_bits(got, want) and got.any()


def test_the_measured_alternatives_compute_the_same(built, tmp_path, monkeypatch):
    """The two forms the A/Bs of csrc/kernels_develop.hip left behind their knobs — k_develop with one lane per pixel, k_develop_tonemap with the
    colour table staged in LDS (5 and the full 1024 entries) — give the default forms' bits."""
    from wave_tracer_amd import Scene, develop
    monkeypatch.setenv("WTGPU_DEVELOP_PER_PIXEL", "1")
    monkeypatch.setenv("WTGPU_TONEMAP_LDS_TABLE", "1")
    for resp, pol, channels, stokes in PLANES:
        sc = Scene.from_xml(_write(tmp_path, f"alt_{channels}_{stokes}.xml", film_xml(response=resp, width=37, height=23, polarimetric=pol))).upload(0)
        films = make_films(23, 37, channels, stokes, 31, "edges")
        d_films = _to_device(sc, films)
        assert same_bits(_host(sc.develop_device(*d_films, 7)), develop(sc, *films, 7))
        for n in (5, 1024):
            tm = {"op": "linear", "mode": "colourmap", "table": random_table(n)}
            for fmt in ("f32", "u8"):
                assert same_bits(_host(sc.tonemap_device(*d_films, 7, tm, stokes - 1, fmt=fmt)), sc.tonemap_host(*films, 7, tm, stokes - 1, fmt=fmt)), (channels, stokes, n, fmt)
