"""Zonal film statistics on the MI355X (wtgpu_film_zonal_device; csrc/kernels_zonal.hip) against the host twin, bit for bit: every count, every bin,
n_outside, min / max, the sum and the painted film.  The sum is exact and order-free (wt/film_zonal.h), so there is nothing to tolerate, in either of
the kernel's two forms — the table in LDS (WTGPU_FILM_ZONAL_LDS=1 wherever it fits 64 KB) and the atomics straight to global memory (0) — or with one
block whose wavefronts take 48 chunks each (WTGPU_FILM_ZONAL_BLOCKS=1).  The host twin itself is held to a numpy / math.fsum restatement by
tests/test_film_zonal.py, whose films and zone plans are used here: P = 1, 3, 4, 12 planes at 37 x 23 (one block, a partial chunk) and at
256 x 192 (48 blocks: the flush crosses blocks)."""
import math

import numpy as np
import pytest

from test_film_stats import F32, PLANES, SPE, checker, option_cases, restate_edges, same_bits, stats_films, stats_scene
from test_film_stats import to_device as _to_device
from test_film_zonal import AXES, FIELDS, PLANS, breaking_films, zone_plan

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (256, 192)]


def _upload(d, P, W, H, monkeypatch_env):
    """an uploaded scene whose knobs were read under monkeypatch_env (the knobs are read once, at the upload)"""
    import os
    old = {k: os.environ.get(k) for k in monkeypatch_env}
    os.environ.update(monkeypatch_env)
    try:
        return stats_scene(d, P, W, H).upload(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    """{(lds, W, H, P)}: both forms at every size and plane count; {("blocks1", lds)}: one block at 256 x 192, RGB"""
    d = tmp_path_factory.mktemp("gpu_film_zonal")
    out = {(lds, W, H, P): _upload(d, P, W, H, {"WTGPU_FILM_ZONAL_LDS": str(lds)}) for lds in (0, 1) for W, H in SIZES for P in PLANES}
    for lds in (0, 1):
        out[("blocks1", lds)] = _upload(d, 3, 256, 192, {"WTGPU_FILM_ZONAL_LDS": str(lds), "WTGPU_FILM_ZONAL_BLOCKS": "1"})
    out["default"] = _upload(d, 3, 256, 192, {})
    return out


def expected_form(lds, Z, planes, bins):
    """The form a call must take (csrc/kernels_zonal.hip: zonal_lds_bytes): the LDS form iff WTGPU_FILM_ZONAL_LDS is not 0 and the edge table plus
    Z x planes entries of nine u64 words, seven u32 counts, two keys and the bins fit the 64 KB a launch may ask for."""
    fits = ((bins + 2) & ~1) * 4 + Z * planes * (9 * 8 + 7 * 4 + 2 * 4 + 4 * bins) <= 64 << 10
    return "lds" if lds and fits else "global"


def _d_zones(sc, zones):
    return _to_device(sc, (zones.view(np.int32),))[0]


def _same(sc, film, d_film, zones, Z, mask, label, spe=SPE, d_mask=None, lds=None, **kw):
    """device = host twin on every field; lds (the scene's WTGPU_FILM_ZONAL_LDS): also that the call took the form it must — both forms give the
    same bits, so a silent fall-back to the global form would show nowhere else"""
    from wave_tracer_amd.api import film_zonal_form
    if mask is not None and d_mask is None:
        d_mask, = _to_device(sc, (mask,))
    got = sc.film_zonal_device(d_film, spe, _d_zones(sc, zones), Z, mask=d_mask, paint=True, **kw)
    if lds is not None:
        planes = sc.spectral_channels + bool(kw.get("luminance"))
        assert film_zonal_form(sc) == expected_form(lds, Z, planes, kw.get("bins", 0)), (label, kw, film_zonal_form(sc))
    want = sc.film_zonal_host(film, spe, zones, Z, mask=mask, paint=True, threads=16, **kw)
    for k in FIELDS:
        assert same_bits(got[k], want[k]), (label, kw, k, np.argwhere(np.asarray(got[k] != want[k]))[:4].tolist())
    assert got["n_outside"] == want["n_outside"] and got["n_zones"] == want["n_zones"] == Z, (label, kw, got["n_outside"], want["n_outside"])
    assert same_bits(got["paint"].cpu().numpy(), want["paint"]), (label, kw, "paint")
    return got


@pytest.mark.parametrize("P", sorted(PLANES))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("lds", [0, 1])
def test_device_equals_host_twin(scenes, lds, size, P):
    """Every plan — Z = 1, 2, 7, one zone per pixel, 65536 sparse — in both forms (where the table does not fit, WTGPU_FILM_ZONAL_LDS=1 is the global
    form too), two of the option cases per plan so that all eight are met."""
    W, H = size
    sc = scenes[(lds, W, H, P)]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    d_mask, = _to_device(sc, (mask,))
    cases = option_cases(channels, stokes)
    for i, plan in enumerate(PLANS):
        zones, Z = zone_plan(plan, H, W, P)
        for k in (i % len(cases), (i + len(cases) // 2) % len(cases)):
            s, abs_, lum, masked = cases[k]
            scale, (lo, hi), bins = AXES[(i + k) % 2]
            films = stats_films(H, W, channels, stokes, 500 + P + k, restate_edges(scale, lo, hi, bins), infinities=bool(k % 2))
            got = _same(sc, films, _to_device(sc, films), zones, Z, mask if masked else None, (lds, W, H, P, plan), d_mask=d_mask if masked else None, lds=lds, stokes_component=s,
                        abs=abs_, luminance=lum, scale=scale, range=(lo, hi), bins=bins)
            assert int(got["n"][:, 0].sum()) + got["n_outside"] == (int((mask > 0).sum()) if masked else W * H) and got["hist"].shape == (Z, channels + lum, bins)
            assert got["n"].any() and (bins == 0 or got["hist"].any())


@pytest.mark.parametrize("lds", [0, 1])
def test_a_table_that_does_not_fit_falls_back(scenes, lds):
    """Z = 300 at four planes: 1200 entries of 108 bytes are beyond the 64 KB a launch may ask for, with or without bins — the call takes the global
    form whatever the knob says; Z = 64 beside it fits."""
    W, H = SIZES[1]
    sc = scenes[(lds, W, H, 3)]
    assert 300 * 4 * 108 > 64 << 10 > 64 * 4 * (108 + 4 * 7)
    rng = np.random.default_rng(12)
    films = stats_films(H, W, 3, 1, 77, restate_edges("dB", -50, 10, 7))
    d_films = _to_device(sc, films)
    for Z in (300, 64):
        zones = rng.integers(0, Z + 3, (H, W)).astype(np.uint32)
        for bins in (0, 7):
            got = _same(sc, films, d_films, zones, Z, None, (lds, Z, bins), lds=lds, luminance=True, scale="dB", range=(-50, 10), bins=bins)
            assert got["n"].all() and got["n_outside"] == int((zones >= Z).sum())
            assert expected_form(lds, Z, 4, bins) == ("lds" if lds and Z == 64 else "global")


@pytest.mark.parametrize("lds", [0, 1])
def test_one_block_takes_the_whole_film(scenes, lds):
    """WTGPU_FILM_ZONAL_BLOCKS=1 at 256 x 192: each of the four wavefronts takes 48 chunks, and the one block's table holds the whole film."""
    W, H = SIZES[1]
    sc = scenes[("blocks1", lds)]
    mask = checker(H, W)
    films = stats_films(H, W, 3, 1, 78, restate_edges("dB", -50, 10, 256))
    d_films = _to_device(sc, films)
    for plan in ("checker", "random7"):
        zones, Z = zone_plan(plan, H, W)
        _same(sc, films, d_films, zones, Z, mask, ("one block", lds, plan), lds=lds, luminance=True, abs=True, scale="dB", range=(-50, 10), bins=256)
    got = _same(sc, films, d_films, np.zeros((H, W), np.uint32), 1, None, ("one block", lds, "one"), scale="dB", range=(-50, 10), bins=256)
    assert (got["n"] == W * H).all()


def test_the_default_rule_computes_the_same(scenes):
    """Without the knob: the LDS form wherever the table fits (checker, random7), the global form where it does not (a zone per pixel)."""
    W, H = SIZES[1]
    sc = scenes["default"]
    films = stats_films(H, W, 3, 1, 79, restate_edges("dB", -50, 10, 256))
    d_films = _to_device(sc, films)
    for plan in ("checker", "random7", "each"):
        zones, Z = zone_plan(plan, H, W)
        bins = 256 if Z * 256 <= 1 << 20 else 7
        _same(sc, films, d_films, zones, Z, checker(H, W), ("default", plan), lds=1, luminance=True, scale="dB", range=(-50, 10), bins=bins)


@pytest.mark.parametrize("lds", [0, 1])
def test_all_equal_elements_in_one_zone(scenes, lds):
    """The most contention there is: every lane of every wavefront adds the same two words of the same zone.  sum == n x, exactly (49152 x has 26
    significant bits)."""
    W, H = SIZES[1]
    sc = scenes[(lds, W, H, 12)]
    x = float(F32(0.1))
    films = (np.full((H, W, 12), x), np.ones((H, W)), np.zeros((H, W, 12)))
    got = _same(sc, films, _to_device(sc, films), np.zeros((H, W), np.uint32), 1, None, ("all equal", lds), lds=lds, spe=0, stokes_component=2, luminance=True, scale="dB",
                range=(-50, 10), bins=64)
    assert (got["n"] == W * H).all() and (got["sum"][0, :3] == W * H * x).all() and (got["min"][0, :3] == F32(x)).all() and (got["max"][0, :3] == F32(x)).all()
    assert (got["hist"][0, :3].sum(axis=1) == W * H).all() and (got["hist"][0, :3] > 0).sum() == 3
    assert (got["paint"].cpu().numpy()[..., :3] == F32(x)).all()


@pytest.mark.parametrize("lds", [0, 1])
def test_films_built_to_break_the_accumulator(scenes, lds):
    """tests/test_film_zonal.py's films — every exponent, full mantissas that straddle words, pairs that cancel, 851 x 3e38, subnormals, NaN payloads,
    infinities — as developed films: device = host twin, which that file holds to math.fsum."""
    W, H = SIZES[0]
    sc = scenes[(lds, W, H, 1)]
    for name, x in breaking_films(H * W).items():
        film = np.ascontiguousarray(x.reshape(H, W, 1, 1))
        d_film, = _to_device(sc, (film,))
        for plan in ("one", "checker", "random7"):
            zones, Z = zone_plan(plan, H, W)
            got = _same(sc, film, d_film, zones, Z, None, (name, plan, lds), lds=lds, spe=None, range=(1.0, 2.0))
            if plan == "one":
                fin = x[np.isfinite(x)]
                assert got["sum"][0, 0] == math.fsum(float(t) for t in fin), name


def test_a_mask_that_excludes_everything(scenes):
    for lds in (0, 1):
        for W, H in SIZES:
            sc = scenes[(lds, W, H, 3)]
            films = stats_films(H, W, 3, 1, 5, restate_edges("dB", -50, 10, 7))
            mask = np.zeros((H, W), F32)
            mask[0, 0] = np.nan
            zones, Z = zone_plan("random7", H, W)
            got = _same(sc, films, _to_device(sc, films), zones, Z, mask, (W, H), luminance=True, scale="dB", range=(-50, 10), bins=7)
            assert not got["n"].any() and not got["hist"].any() and got["n_outside"] == 0 and same_bits(got["sum"], np.zeros((Z, 4)))
            assert np.isnan(got["min"]).all() and np.isnan(got["max"]).all() and not got["paint"].any().item()


def test_both_source_kinds(scenes):
    """A developed film on the device gives what its accumulators give (and what the host twin gives of either)."""
    W, H = SIZES[1]
    for lds, P in ((0, 12), (1, 3)):
        sc = scenes[(lds, W, H, P)]
        _, _, channels, stokes = PLANES[P]
        films = stats_films(H, W, channels, stokes, 90 + P, restate_edges("dB", -50, 10, 7))
        d_films = _to_device(sc, films)
        d_developed = sc.develop_device(*d_films, SPE)
        developed = d_developed.cpu().numpy()
        zones, Z = zone_plan("random7", H, W)
        kw = dict(stokes_component=stokes - 1, luminance=True, scale="dB", range=(-50, 10), bins=7)
        a = _same(sc, films, d_films, zones, Z, checker(H, W), ("accumulators", P), **kw)
        b = _same(sc, developed, d_developed, zones, Z, checker(H, W), ("developed", P), spe=None, **kw)
        assert all(same_bits(a[k], b[k]) for k in FIELDS) and same_bits(a["paint"].cpu().numpy(), b["paint"].cpu().numpy())


def _against_masked_stats(sc, d_films, spe, d_zones, Z, got, **kw):
    """A zone's record against film_stats_device with the zone as the mask: counts, bins and extrema bit for bit; the sums differ by construction
    (that one is the pairwise f64 sum) and are held to n 2^-52 sum|x|, the bound of f64 addition in any order."""
    for zone in range(Z):
        d_m = (d_zones == zone).float().contiguous()
        st = sc.film_stats_device(*d_films, spe, mask=d_m, **kw)
        sa = sc.film_stats_device(*d_films, spe, mask=d_m, **dict(kw, abs=True))
        for k in ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above", "min", "max"):
            assert same_bits(got[k][zone], st[k]), (zone, k, got[k][zone], st[k])
        assert np.array_equal(got["hist"][zone], st["hist"])
        assert not got["n_inf"][zone].any() and not got["n_nan"][zone].any()
        for c in range(len(st["sum"])):
            assert abs(got["sum"][zone, c] - st["sum"][c]) <= float(st["n"][c]) * 2.0 ** -52 * float(sa["sum"][c]) * (1 + 1e-9), (zone, c, got["sum"][zone, c], st["sum"][c])


def test_rendered_scenes(built):
    """The bundled etoile at res 64 with line_of_sight's n_visible as the zones, against one masked film_stats_device call per zone; cornell_box
    under first_hit's shape ids, device against host twin."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films, coverage_by_los, view
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    sc = Scene("etoile", res=64, mesh_detail=0).upload(0)
    d_films = alloc_films(sc, dev)
    sc.render_into(*d_films, 0, 4, 21, st)
    torch.cuda.synchronize(dev)
    films = tuple(t.cpu().numpy() for t in d_films)
    d_zones = sc.line_of_sight(0, 1, maps=(), ids=("n_visible",))["n_visible"].contiguous()
    zones = d_zones.cpu().numpy().view(np.uint32)
    kw = dict(scale="dB", range=(-120.0, 0.0), bins=64, luminance=sc.spectral_channels == 3)
    got = sc.film_zonal_device(d_films, 4, d_zones, **kw)
    Z = got["n_zones"]
    assert Z == int(zones.max()) + 1 >= 2 and got["n"].all() and got["n_outside"] == 0 and got["sum"].any()
    want = sc.film_zonal_host(films, 4, zones, **kw)
    assert all(same_bits(got[k], want[k]) for k in FIELDS)
    _against_masked_stats(sc, d_films, 4, d_zones, Z, got, **kw)
    by_los = coverage_by_los(sc, d_films, 4, **kw)
    assert by_los["n_zones"] == 2 and np.array_equal(by_los["n"][0], got["n"][0]) and by_los["n"][:, 0].sum() == sc.width * sc.height
    box = Scene("cornell_box", res=64, mesh_detail=1).upload(0)
    d_films = alloc_films(box, dev)
    box.render_into(*d_films, 0, 4, 22, st)
    torch.cuda.synchronize(dev)
    d_shape = box.first_hit(0, 1, maps=(), ids=("shape",))["shape"].contiguous()
    shape = d_shape.cpu().numpy().view(np.uint32)
    films = tuple(t.cpu().numpy() for t in d_films)
    kw = dict(luminance=True, scale="dB", range=(-60.0, 20.0), bins=32, paint=True)
    got = box.film_zonal_device(d_films, 4, d_shape, **kw)
    want = box.film_zonal_host(films, 4, shape, **kw)
    assert got["n_zones"] == int(shape[shape != 0xFFFFFFFF].max()) + 1 > 2 and got["n_outside"] == int((shape == 0xFFFFFFFF).sum())
    assert all(same_bits(got[k], want[k]) for k in FIELDS) and same_bits(got["paint"].cpu().numpy(), want["paint"]) and got["sum"].any()
    # the painted zone means are a developed film: render.view shows them
    picture = view(box, got["paint"][..., :3].contiguous().reshape(box.height, box.width, 3, 1))
    assert tuple(picture.shape) == (box.height, box.width, 3) and picture.any().item()


def test_zonal_between_renders_changes_nothing(built):
    """As test_gpu_film_stats.py's: the calls count nothing and leave the films they read alone."""
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import cell_zones
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_films = _to_device(sc, a)
    zones, Z = cell_zones(sc.height, sc.width, 8)
    got = sc.film_zonal_device(d_films, 2, _d_zones(sc, zones), Z, luminance=sc.spectral_channels == 3, paint=True)
    assert all(v == 0 for v in sc.counters().values()) and got["n"].sum() == sc.width * sc.height * got["n"].shape[1]
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_films))


def test_refusals_on_the_device_side(scenes, tmp_path):
    """A scene that is not uploaded: WTGPU_ERR_INVALID (1) from the entry point itself, with the message, and the Python method says the same before
    it gets there; zones of another dtype, shape or device are refused in Python."""
    import ctypes as C
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FILM_ZONAL_FIELDS, FilmSource, FilmZonalSpec, film_zonal_form, load_library
    sc = stats_scene(tmp_path, 1)
    dev = torch.device("cuda", 0)
    v, w, l = (torch.zeros(37 * 23, dtype=torch.float64, device=dev) for _ in range(3))
    z = torch.zeros((23, 37), dtype=torch.int32, device=dev)
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_zonal_device((v, w, l), 1, z, 1)
    assert film_zonal_form(sc) is None      # no call has launched anything
    lib = load_library()
    src, spec, n_out = FilmSource(v.data_ptr(), w.data_ptr(), l.data_ptr(), 1, None), FilmZonalSpec(0, 0, 0, 0, 1, 0.0, 0.0), C.c_uint64(0)
    rec = np.zeros((1, 1), np.dtype(FILM_ZONAL_FIELDS))
    rc = lib.wtgpu_film_zonal_device(sc.handle, None, C.byref(src), C.byref(spec), z.data_ptr(), None, rec.ctypes.data, None, C.byref(n_out), None)
    assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
    up = scenes[(1, 37, 23, 1)]
    for bad in (z.long(), z[:, :-1], z.cpu(), z.t().contiguous().t()):
        with pytest.raises(ValueError, match="zones: a contiguous torch.int32"):
            up.film_zonal_device((v, w, l), 1, bad, 1)
    with pytest.raises(WtgpuError, match=r"n_zones 65537 out of range"):
        up.film_zonal_device((v, w, l), 1, z, 65537)
