"""Zonal film statistics (wt/film_zonal.h: wtgpu_film_zonal_host; render.zones_from_edges, cell_zones, zonal, coverage_by_los) on the CPU: the host
twin against a numpy / Python restatement written here (it calls nothing of the library), on the synthetic films of tests/test_film_stats.py, whose
developed values are known exactly, and on films built to break the accumulator.  tests/test_gpu_film_zonal.py runs the device kernels against the
host twin on the same films and zone plans.

What must agree exactly: every count, every bin, n_outside, min / max (bit for bit, -0 below +0) and the sum — the exact sum of the zone's finite
elements rounded once, which is math.fsum of them as floats: an oracle nobody here wrote.  Against the film statistics with the zone as the mask
the counts, bins and extrema are the same bits; the two sums differ by construction (that one is a pairwise f64 sum) and are held to
n 2^-52 sum|x|, the bound tests/test_film_stats.py derives for f64 addition in any order."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_film_stats import (F32, H, PLANES, SPE, W, checker, elements, option_cases, restate_edges, restate_stats, same_bits, stats_films, stats_scene)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ZONE = 0xFFFFFFFF
COUNTS = ("n", "n_nan", "n_inf", "n_negative", "n_zero", "n_below", "n_above")
FIELDS = COUNTS + ("min", "max", "sum", "hist", "edges", "mean")
PLANS = ("one", "checker", "random7", "each", "sparse")
AXES = (("dB", (-50.0, 10.0), 7), ("linear", (0.25, 3.0), 0))      # (scale, range, bins): with bins, and the one edge that splits below from above


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_zonal")
    return {P: stats_scene(d, P) for P in PLANES}


# ---- zone plans -------------------------------------------------------------------------------------------------------------------------------
def zone_plan(name, height, width, seed=0):
    """(zones uint32 [height, width], n_zones): Z = 1; Z = 2 from a checker; Z = 7 random with ids >= Z and 0xFFFFFFFF present; one pixel per zone
    (851 at 37 x 23); Z = 65536, sparse, with zones 0 and 65535 and ids beyond."""
    rng = np.random.default_rng(1000 + seed)
    n = height * width
    yy, xx = np.mgrid[0:height, 0:width]
    if name == "one":
        return np.zeros((height, width), np.uint32), 1
    if name == "checker":
        return ((yy + xx) % 2).astype(np.uint32), 2
    if name == "random7":
        z = rng.integers(0, 10, n).astype(np.uint32)        # 7, 8, 9: outside
        z[rng.random(n) < 0.1] = NO_ZONE
        z[:4] = [6, 7, NO_ZONE, 0]
        return z.reshape(height, width), 7
    if name == "each":
        assert n <= 65536
        return rng.permutation(n).astype(np.uint32).reshape(height, width), n
    if name == "sparse":
        z = rng.integers(0, 65536, n).astype(np.uint32)
        z[rng.random(n) < 0.05] = NO_ZONE
        z[:6] = [0, 65535, 65536, NO_ZONE, 65535, 1 << 31]
        return z.reshape(height, width), 65536
    raise KeyError(name)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------
def restate_zonal(x, edges, mask, zones, n_zones):
    """x: [pixels, planes] f32 -> the statistics Scene.film_zonal_host returns, zone by zone through test_film_stats.restate_stats with the zone's
    pixels as the mask; n_inf and the sum — math.fsum over the zone's finite elements as floats — are stated here."""
    planes, bins = x.shape[1], len(edges) - 1
    inc = np.ones(len(x), bool) if mask is None else (mask.reshape(-1) > 0)
    z = zones.reshape(-1).astype(np.uint32).astype(np.int64)
    member = inc & (z < n_zones)
    out = {k: np.zeros((n_zones, planes), np.uint64) for k in COUNTS}
    out.update(min=np.full((n_zones, planes), np.nan, F32), max=np.full((n_zones, planes), np.nan, F32), sum=np.zeros((n_zones, planes), np.float64),
               hist=np.zeros((n_zones, planes, bins), np.uint64), n_outside=int((inc & ~member).sum()))
    for zone in np.unique(z[member]):
        sel = member & (z == zone)
        r = restate_stats(x, edges, sel.astype(F32))
        for k in COUNTS:
            if k != "n_inf":
                out[k][zone] = r[k]
        out["min"][zone], out["max"][zone] = r["min"], r["max"]
        out["hist"][zone] = np.array(r["hist"], dtype=np.uint64).reshape(planes, bins)
        for c in range(planes):
            v = x[sel, c]
            out["n_inf"][zone, c] = int(np.isinf(v).sum())
            out["sum"][zone, c] = math.fsum(float(t) for t in v[np.isfinite(v)]) + 0.0      # (+ 0.0: fsum of nothing is 0.0 already; an exact zero is +0.0)
    return out


def check_zonal(got, want, label):
    for k in COUNTS:
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], want[k]), (label, k)
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"]), (label, "hist")
    assert got["n_outside"] == want["n_outside"], (label, "n_outside", got["n_outside"], want["n_outside"])
    for k in ("min", "max"):
        assert same_bits(got[k], want[k].astype(F32)), (label, k)
    assert same_bits(got["sum"], want["sum"]), (label, "sum against math.fsum", got["sum"][got["sum"] != want["sum"]][:4], want["sum"][got["sum"] != want["sum"]][:4])


def same_result(a, b, label):
    for k in FIELDS:
        assert same_bits(a[k], b[k]), (label, k)
    assert a["n_outside"] == b["n_outside"] and a["n_zones"] == b["n_zones"], label
    assert ("paint" in a) == ("paint" in b) and ("paint" not in a or same_bits(np.asarray(a["paint"]), np.asarray(b["paint"]))), (label, "paint")


# ---- the host twin against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("P", sorted(PLANES))
def test_host_twin_equals_the_restatement(scenes, P, plan):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    zones, Z = zone_plan(plan, H, W, P)
    cases = option_cases(channels, stokes)
    if Z > 7:       # the large plans: with and without everything, not all eight combinations
        cases = [cases[0], cases[-1]]
    for k, (s, abs_, lum, masked) in enumerate(cases):
        scale, (lo, hi), bins = AXES[k % 2]
        edges = restate_edges(scale, lo, hi, bins)
        films = stats_films(H, W, channels, stokes, 300 + P + k, edges, infinities=bool(k % 3))
        m = mask if masked else None
        got = sc.film_zonal_host(films, SPE, zones, Z, stokes_component=s, abs=abs_, luminance=lum, mask=m, scale=scale, range=(lo, hi), bins=bins, threads=3)
        label = (P, plan, s, abs_, lum, masked, scale, bins)
        assert got["n_zones"] == Z and got["hist"].shape == (Z, channels + lum, bins) and same_bits(got["edges"], edges), label
        want = restate_zonal(elements(channels, stokes, films, SPE, s, abs_, lum), edges, m, zones, Z)
        check_zonal(got, want, label)
        assert int(got["n"][:, 0].sum()) + got["n_outside"] == (H * W if m is None else int((m > 0).sum())), label
        if plan == "one" and not masked and not lum:     # the film was built to meet every class
            assert got["n_nan"].all() and got["n_zero"].all() and got["n_above"].all() and (abs_ or got["n_negative"].all()) and (not k % 3 or got["n_inf"].all()), label


def test_n_zones_none_takes_the_largest_id(scenes):
    sc = scenes[3]
    films = stats_films(H, W, 3, 1, 1, restate_edges("dB", -50, 10, 4))
    zones, _ = zone_plan("random7", H, W)
    got = sc.film_zonal_host(films, SPE, zones)
    assert got["n_zones"] == 10 and got["n"].shape == (10, 3) and got["n_outside"] == int((zones == NO_ZONE).sum())
    assert sc.film_zonal_host(films, SPE, zones.view(np.int32))["n_zones"] == 10         # the id maps are int32 holding the u32 bits
    assert sc.film_zonal_host(films, SPE, np.full((H, W), NO_ZONE, np.uint32))["n_zones"] == 1
    with pytest.raises(ValueError, match="more than 65536 zones"):
        sc.film_zonal_host(films, SPE, zone_plan("sparse", H, W)[0])


# ---- films built to break the accumulator -----------------------------------------------------------------------------------------------------
def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(F32)


def breaking_films(n=H * W, seed=5):
    """{name: f32[n]}: developed elements for a one-plane film."""
    rng = np.random.default_rng(seed)
    out = {}
    e = np.arange(255, dtype=np.uint32)
    x = np.zeros(n, F32)
    x[:255] = _bits(e << 23 | rng.integers(0, 1 << 23, 255).astype(np.uint32) | (rng.integers(0, 2, 255).astype(np.uint32) << 31))
    out["every exponent"] = rng.permutation(x)
    x = np.zeros(n, F32)
    x[:254] = _bits((e[1:] << 23) | np.uint32(0x7FFFFF))                       # m = 0xFFFFFF at every sh, so every sh & 31: the addend straddles two words
    x[254:508] = -x[:254][::-1] * F32(0.5)
    out["full mantissas"] = x
    half = (n - 1) // 2
    v = _bits(rng.integers(0, 0x7F800000, half).astype(np.uint32))
    x = np.zeros(n, F32)
    x[:half], x[half:2 * half], x[2 * half] = v, -v, F32(1e-45)
    out["pairs that cancel"] = rng.permutation(x)
    out["851 x 3e38"] = np.full(n, 3e38, F32)
    out["all equal"] = np.full(n, 0.1, F32)
    x = _bits(rng.integers(0, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))      # subnormals of both signs
    x[:8] = [-0.0, 0.0, np.inf, -np.inf, np.inf, 1e-45, -1e-45, 1.0]
    x[8:12] = _bits([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF])                                                  # NaNs with payloads
    out["subnormals and specials"] = x
    return out


def test_films_built_to_break_the_accumulator(scenes):
    sc = scenes[1]
    edges = restate_edges("linear", 1.0, 2.0, 0)
    for name, x in breaking_films().items():
        film = np.ascontiguousarray(x.reshape(H, W, 1, 1))
        for plan in ("one", "checker"):
            zones, Z = zone_plan(plan, H, W)
            got = sc.film_zonal_host(film, None, zones, Z, range=(1.0, 2.0), threads=2)
            check_zonal(got, restate_zonal(x.reshape(-1, 1), edges, None, zones, Z), (name, plan))
        one = sc.film_zonal_host(film, None, np.zeros((H, W), np.uint32), 1, range=(1.0, 2.0))
        if name == "pairs that cancel":
            assert one["sum"][0, 0] == 1.401298464324817e-45
        if name == "851 x 3e38":
            assert one["sum"][0, 0] == 851 * float(F32(3e38)) and one["sum"][0, 0] > 3.4e38 * 700
        if name == "all equal":
            assert one["sum"][0, 0] == math.fsum([float(F32(0.1))] * 851) and one["min"][0, 0] == one["max"][0, 0] == F32(0.1)
        if name == "subnormals and specials":
            assert one["n_inf"][0, 0] == 3 and one["n_nan"][0, 0] == 4 and np.isinf(one["max"][0, 0]) and np.isinf(one["min"][0, 0])


def _words_value(words):
    return sum((int(w) - (1 << 64 if int(w) >> 63 else 0)) << (32 * k) for k, w in enumerate(words))


def test_fz_round_on_hand_made_words(built):
    """Python's int / int division is correctly rounded: the oracle of fz_round for any nine words."""
    from wave_tracer_amd.api import fz_sum
    u64 = lambda v: v & ((1 << 64) - 1)
    cases = {
        "tie to even, down": [u64((1 << 53) + 1), 0, 0, 0, 0, 0, 0, 0, 0],
        "tie to even, up": [u64((1 << 53) + 3), 0, 0, 0, 0, 0, 0, 0, 0],
        "above the tie by the lowest bit": [1, u64((1 << 53) + 1) << 5 & ((1 << 64) - 1), 0, 0, 0, 0, 0, 0, 0],
        "a carry out of the 53 bits": [u64((1 << 54) - 1), 0, 0, 0, 0, 0, 0, 0, 0],
        "the same, negative": [u64(-((1 << 54) - 1)), 0, 0, 0, 0, 0, 0, 0, 0],
        "an exact zero from non-zero words": [1 << 32, u64(-1), 0, 0, 0, 0, 0, 0, 0],
        "a zero across all words": [1 << 32] + [u64((1 << 32) - 1)] * 7 + [u64(-1)],
        "a negative carry through all words": [u64(-1), 0, 0, 0, 0, 0, 0, 0, 1],
        "one unit": [1, 0, 0, 0, 0, 0, 0, 0, 0],
    }
    rng = np.random.default_rng(3)
    for i in range(200):
        w = [int(t) for t in rng.integers(0, 1 << 64, 9, dtype=np.uint64)]
        top = int(rng.integers(0, 9))
        w[top] = u64(int(rng.integers(-(1 << 31), 1 << 31)))          # a small top word, zeros above it: totals of every magnitude
        w[top + 1:] = [0] * (8 - top)
        cases[f"random {i}"] = w
    for name, words in cases.items():
        got, after = fz_sum((), words)
        v = _words_value(words)
        want = v / (1 << 149) if v else 0.0
        assert same_bits(np.float64(got), np.float64(want)), (name, got, want)
        assert after.tolist() == [int(t) for t in words]
    assert fz_sum((), cases["tie to even, down"])[0] == 2.0 ** (53 - 149) and fz_sum((), cases["tie to even, up"])[0] == (2.0 ** 53 + 4) * 2.0 ** -149
    assert math.copysign(1.0, fz_sum((), cases["an exact zero from non-zero words"])[0]) == 1.0


def test_exact_sum_equals_fsum_over_the_whole_exponent_range(built):
    from wave_tracer_amd.api import fz_sum
    rng = np.random.default_rng(11)
    for draw in range(200):
        n = int(rng.integers(1, 400))
        x = _bits(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        if draw % 3 == 0:
            x = np.concatenate((x, -x, _bits(rng.integers(0, 1 << 23, 3).astype(np.uint32))))     # cancellations with subnormals left over
        if draw % 5 == 0:
            x = np.concatenate((x, np.full(40, 3e38, F32), np.full(39, -3e38, F32)))
        fin = x[np.isfinite(x)]
        got, _ = fz_sum(rng.permutation(x))
        assert same_bits(np.float64(got), np.float64(math.fsum(float(t) for t in fin) + 0.0)), draw


# ---- against the film statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 12])
def test_a_zone_equals_the_film_statistics_with_the_zone_as_the_mask(scenes, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    lo, hi = -50.0, 10.0
    edges = restate_edges("dB", lo, hi, 256)
    mask = checker(H, W)
    for plan in ("checker", "random7"):
        zones, Z = zone_plan(plan, H, W)
        for infinities in (False, True):
            films = stats_films(H, W, channels, stokes, 40 + P, edges, infinities)
            kw = dict(stokes_component=stokes - 1, abs=True, luminance=True, scale="dB", range=(lo, hi), bins=256)
            got = sc.film_zonal_host(films, SPE, zones, Z, mask=mask, **kw)
            x = elements(channels, stokes, films, SPE, stokes - 1, True, True)
            for zone in range(Z):
                zmask = np.where((mask > 0) & (zones == zone), F32(1), F32(0))
                st = sc.film_stats_host(*films, SPE, mask=zmask, **kw)
                for k in ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above", "min", "max"):
                    assert same_bits(got[k][zone], st[k]), (P, plan, zone, k)
                assert np.array_equal(got["hist"][zone], st["hist"]) and same_bits(got["edges"], st["edges"])
                if not infinities:      # (the statistics' sum takes the infinities in; the zonal sum is over the finite elements)
                    for c in range(channels + 1):
                        v = x[zmask.reshape(-1) > 0, c]
                        v = v[~np.isnan(v)].astype(np.float64)
                        assert abs(got["sum"][zone, c] - st["sum"][c]) <= len(v) * 2.0 ** -52 * math.fsum(np.abs(v)), (P, plan, zone, c)
                else:
                    assert got["n_inf"].any()


# ---- further checks ---------------------------------------------------------------------------------------------------------------------------
def test_a_developed_source_equals_the_accumulators(scenes):
    from wave_tracer_amd.render import develop
    for P in (3, 12):
        sc = scenes[P]
        _, _, channels, stokes = PLANES[P]
        films = stats_films(H, W, channels, stokes, 60 + P, restate_edges("dB", -50, 10, 7))
        developed = develop(sc, *films, SPE).reshape(H, W, channels, stokes)
        zones, Z = zone_plan("random7", H, W)
        kw = dict(stokes_component=stokes - 1, luminance=True, mask=checker(H, W), scale="dB", range=(-50, 10), bins=7, paint=True)
        same_result(sc.film_zonal_host(films, SPE, zones, Z, **kw), sc.film_zonal_host(developed, None, zones, Z, **kw), P)


def test_the_result_does_not_depend_on_the_threads(scenes):
    for P in (3, 12):
        _, _, channels, stokes = PLANES[P]
        films = stats_films(H, W, channels, stokes, 9, restate_edges("dB", -50, 10, 256))
        for plan in ("random7", "each"):
            zones, Z = zone_plan(plan, H, W)
            a, b = (scenes[P].film_zonal_host(films, SPE, zones, Z, scale="dB", range=(-50, 10), bins=256, luminance=True, mask=checker(H, W), paint=True, threads=t)
                    for t in (1, 5))
            same_result(a, b, (P, plan))


def test_paint_is_the_zone_mean(scenes):
    sc = scenes[3]
    films = stats_films(H, W, 3, 1, 21, restate_edges("dB", -50, 10, 4), infinities=True)
    mask = checker(H, W)
    for plan in ("checker", "random7", "each"):
        zones, Z = zone_plan(plan, H, W)
        for m in (None, mask):
            got = sc.film_zonal_host(films, SPE, zones, Z, luminance=True, mask=m, paint=True)
            n_fin = (got["n"] - got["n_nan"] - got["n_inf"]).astype(np.float64)
            with np.errstate(all="ignore"):
                mean = np.where(n_fin > 0, (got["sum"] / n_fin).astype(F32), F32(0))
            assert np.array_equal(got["mean"], got["sum"] / np.where(n_fin > 0, n_fin, np.nan), equal_nan=True)
            inc = (np.ones((H, W), bool) if m is None else m > 0) & (zones < Z)
            want = np.where(inc[..., None], mean[np.where(inc, zones, 0)], F32(0)).astype(F32)
            assert got["paint"].shape == (H, W, 4) and same_bits(got["paint"], want), plan
            assert (got["paint"][~inc] == 0).all() and got["paint"].any()
    # a zone whose elements are all NaN or infinite is painted 0
    film = np.full((H, W, 3, 1), np.nan, F32)
    film[0] = np.inf
    got = sc.film_zonal_host(film, None, np.zeros((H, W), np.uint32), 1, paint=True)
    assert not got["paint"].any() and (got["sum"] == 0).all() and (got["n_inf"] == W).all() and np.isnan(got["mean"]).all()


def test_refusals_say_why(scenes):
    import ctypes as C
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FILM_ZONAL_FIELDS, FilmSource, FilmZonalSpec, load_library
    mono, rgb = scenes[1], scenes[3]
    fm, fr = stats_films(H, W, 1, 1, 1, restate_edges("dB", -50, 10, 4)), stats_films(H, W, 3, 1, 1, restate_edges("dB", -50, 10, 4))
    zones = np.zeros((H, W), np.uint32)
    # everything the film statistics refuse, in their words
    with pytest.raises(WtgpuError, match=r"film_zonal: stokes_component 1 out of range \(the film has 1\)"):
        mono.film_zonal_host(fm, SPE, zones, 1, stokes_component=1)
    with pytest.raises(WtgpuError, match="film_zonal: bins 4097 above the 4096"):
        rgb.film_zonal_host(fr, SPE, zones, 1, range=(-50, 10), bins=4097)
    with pytest.raises(WtgpuError, match="film_zonal: lo < hi expected with bins > 0"):
        rgb.film_zonal_host(fr, SPE, zones, 1, range=(10, -50), bins=8)
    with pytest.raises(WtgpuError, match="film_zonal: a finite range expected"):
        rgb.film_zonal_host(fr, SPE, zones, 1, range=(-50, float("inf")), bins=8)
    with pytest.raises(WtgpuError, match=r"film_zonal: LUMINANCE needs a 3-channel film \(this one has 1\)"):
        mono.film_zonal_host(fm, SPE, zones, 1, luminance=True)
    with pytest.raises(WtgpuError, match=r"film_zonal: degenerate edges: edge 1 of 256 is not above edge 0"):
        rgb.film_zonal_host(fr, SPE, zones, 1, range=(1.0, float(np.nextafter(F32(1), F32(2)))), bins=256)
    # the zones'
    for Z in (0, 65537):
        with pytest.raises(WtgpuError, match=rf"film_zonal: n_zones {Z} out of range \(1 .. 65536\)"):
            rgb.film_zonal_host(fr, SPE, zones, Z)
    with pytest.raises(WtgpuError, match=r"film_zonal: n_zones x bins = 1052672 above the 1048576"):
        rgb.film_zonal_host(fr, SPE, zones, 4112, range=(-50, 10), scale="dB", bins=256)
    assert rgb.film_zonal_host(fr, SPE, zones, 4096, range=(-50, 10), scale="dB", bins=256)["hist"].shape == (4096, 3, 256)
    # in Python: dtype, shape, scale, bins without a range
    with pytest.raises(ValueError, match="zones: a contiguous int32 or uint32 array"):
        rgb.film_zonal_host(fr, SPE, zones.astype(np.int64), 1)
    with pytest.raises(ValueError, match="zones: a contiguous int32 or uint32 array"):
        rgb.film_zonal_host(fr, SPE, zones[:, :-1], 1)
    with pytest.raises(ValueError, match="scale"):
        rgb.film_zonal_host(fr, SPE, zones, 1, scale="log")
    with pytest.raises(ValueError, match="bins > 0 needs a range"):
        rgb.film_zonal_host(fr, SPE, zones, 1, bins=8)
    with pytest.raises(ValueError, match="films of the scene's size"):
        rgb.film_zonal_host(fm, SPE, zones, 1)
    # at the entry point itself: missing planes and results, a source that is no source
    lib = load_library()
    v, w, l = (np.ascontiguousarray(t) for t in fr)
    src = FilmSource(v.ctypes.data, w.ctypes.data, l.ctypes.data, SPE, None)
    spec, rec, hist, n_out = FilmZonalSpec(0, 0, 0, 0, 1, 0.0, 0.0), np.zeros((1, 3), np.dtype(FILM_ZONAL_FIELDS)), np.zeros(3 * 8, np.uint64), C.c_uint64(0)

    def call(src=src, spec=spec, zones=zones.ctypes.data, out=rec.ctypes.data, hist=None, n_out=C.byref(n_out)):
        rc = lib.wtgpu_film_zonal_host(rgb.handle, C.byref(src), C.byref(spec), zones, None, 1, out, hist, n_out, None)
        return rc, lib.wtgpu_last_error().decode()
    assert call()[0] == 0
    assert call(zones=None) == (1, "film_zonal: a zone plane expected (zones is NULL)")
    assert call(out=None) == (1, "film_zonal: out and n_outside expected (one of them is NULL)")
    assert call(n_out=None) == (1, "film_zonal: out and n_outside expected (one of them is NULL)")
    assert call(spec=FilmZonalSpec(0, 1, 8, 0, 1, -50.0, 10.0)) == (1, "film_zonal: bins > 0 without a histogram (hist is NULL)")
    assert call(spec=FilmZonalSpec(0, 1, 8, 0, 1, -50.0, 10.0), hist=hist.ctypes.data)[0] == 0
    assert call(spec=FilmZonalSpec(0, 2, 0, 0, 1, 0.0, 0.0)) == (1, "film_zonal: scale 0 (linear) or 1 (dB) expected")
    assert call(spec=FilmZonalSpec(0, 0, 0, 4, 1, 0.0, 0.0)) == (1, "film_zonal: flags 1 (ABS) and 2 (LUMINANCE) expected")
    rc, msg = call(src=FilmSource(v.ctypes.data, None, l.ctypes.data, SPE, None))
    assert rc == 1 and msg.startswith("film_zonal: film source: the accumulators are value, weight and light together")
    rc, msg = call(src=FilmSource(None, None, None, 0, None))
    assert rc == 1 and msg.startswith("film_zonal: film source: neither form is set")


def test_a_film_of_2_to_the_31_pixels_is_refused(built, tmp_path):
    """The guard behind "no word overflows whatever the order": a word gains less than 2^32 per element, so 2^31 elements are one too many.  A scene
    holds nothing per pixel, and the entry point refuses before it reads a plane, so the pointers here only have to be non-null.  65536 x 32768
    is refused; 65536 x 32767 passes this check — the next refusal in line (bins without a histogram) is what answers."""
    import ctypes as C
    from wave_tracer_amd.api import FILM_ZONAL_FIELDS, FilmSource, FilmZonalSpec, load_library
    lib = load_library()
    dummy = np.zeros(64, np.float64)
    rec, n_out = np.zeros((1, 1), np.dtype(FILM_ZONAL_FIELDS)), C.c_uint64(7)
    for source in (FilmSource(dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data, SPE, None), FilmSource(None, None, None, 0, dummy.ctypes.data)):
        for height, refused in ((32768, True), (32767, False)):
            sc = stats_scene(tmp_path, 1, 65536, height)
            assert sc.width * sc.height == (1 << 31) - (0 if refused else 65536)
            for bins, hist in ((0, None), (8, None)) if refused else ((8, None),):      # (a call that passed every check would read the planes)
                spec = FilmZonalSpec(0, 1, bins, 0, 1, -50.0, 10.0)
                rc = lib.wtgpu_film_zonal_host(sc.handle, C.byref(source), C.byref(spec), dummy.ctypes.data, None, 1, rec.ctypes.data, hist, C.byref(n_out), None)
                msg = lib.wtgpu_last_error().decode()
                if refused:
                    assert (rc, msg) == (1, "film_zonal: a film of 2^31 pixels or more (a word of the exact sum could overflow)"), (height, bins, rc, msg)
                else:
                    assert (rc, msg) == (1, "film_zonal: bins > 0 without a histogram (hist is NULL)"), (height, bins, rc, msg)
            assert n_out.value == 7 and not rec["n"].any()      # nothing was written


# ---- the helpers ------------------------------------------------------------------------------------------------------------------------------
def test_zones_from_edges(built):
    import torch
    from wave_tracer_amd.render import NO_ZONE as no_zone, zones_from_edges
    edges = [1.0, 2.0, 4.0, 8.0]
    e = np.array(edges, F32)
    x = np.array([[0.5, 1.0, np.nextafter(F32(2), F32(0)), 2.0], [4.0, np.nextafter(F32(8), F32(0)), 8.0, np.nan], [np.inf, -np.inf, -0.0, 3.0]], F32)
    want = np.array([[no_zone, 0, 0, 1], [2, 2, no_zone, no_zone], [no_zone, no_zone, no_zone, 1]], np.uint32)
    got = zones_from_edges(x, edges)
    assert no_zone == NO_ZONE and got.dtype == np.uint32 and np.array_equal(got, want)
    t = zones_from_edges(torch.from_numpy(x), e)
    assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), want)
    rng = np.random.default_rng(4)
    big = (10.0 ** rng.uniform(-1, 1.2, (H, W))).astype(F32)
    z = zones_from_edges(big, edges)
    for i in range(3):
        assert np.array_equal(z == i, (big >= e[i]) & (big < e[i + 1]))
    with pytest.raises(ValueError, match="strictly increasing"):
        zones_from_edges(x, [1.0, 1.0])


def test_cell_zones(built):
    from wave_tracer_amd.render import cell_zones
    z, n = cell_zones(H, W, 8)
    assert z.dtype == np.uint32 and z.shape == (H, W) and n == 3 * 5 and z[0, 0] == 0 and z[7, 7] == 0 and z[8, 0] == 5 and z[0, 8] == 1 and z[H - 1, W - 1] == 14
    assert np.bincount(z.reshape(-1)).tolist()[:5] == [64, 64, 64, 64, 8 * 5] and cell_zones(H, W, 64)[1] == 1
    with pytest.raises(ValueError):
        cell_zones(H, W, 0)


def test_zonal_and_its_percentiles(scenes):
    """render.zonal on numpy films: block averages over 8 x 8 cells, and per-zone percentiles that are imageio.percentiles of the film statistics
    with the zone as the mask."""
    from wave_tracer_amd import imageio
    from wave_tracer_amd.render import cell_zones, zonal
    sc = scenes[1]
    films = stats_films(H, W, 1, 1, 33, restate_edges("dB", -50, 10, 256), infinities=False)
    zones, Z = cell_zones(H, W, 8)
    st = zonal(sc, films, SPE, zones, Z, scale="dB", range=(-50, 10), bins=256)
    assert st["n"].shape == (15, 1) and st["n"].sum() == H * W and st["n_outside"] == 0
    p = st.percentiles([10, 50, 90])
    assert p.shape == (15, 1, 3) and st.percentiles(50).shape == (15, 1)
    for zone in (0, 7, 14):
        ref = sc.film_stats_host(*films, SPE, mask=(zones == zone).astype(F32), scale="dB", range=(-50, 10), bins=256)
        assert np.array_equal(p[zone], imageio.percentiles(ref, [10, 50, 90]), equal_nan=True)
    with pytest.raises(ValueError, match="percentiles need a histogram"):
        zonal(sc, films, SPE, zones, Z).percentiles(50)


def test_coverage_by_los_is_the_two_zone_call(built):
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import coverage_by_los, los_masks, zonal
    sc = Scene("etoile", res=32, mesh_detail=0)
    rng = np.random.default_rng(8)
    films = (rng.uniform(0, 2, (sc.height, sc.width, sc.channels)), np.ones((sc.height, sc.width)), np.zeros((sc.height, sc.width, sc.channels)))
    got = coverage_by_los(sc, films, 1)
    los, nlos = los_masks(sc, host=True)
    assert got["n_zones"] == 2 and got["n_outside"] == 0 and got["n"][:, 0].tolist() == [int(nlos.sum()), int(los.sum())] and got["n"].all()
    same_result(got, zonal(sc, films, 1, (los > 0).astype(np.uint32), 2), "coverage_by_los")
    for zone, m in ((0, nlos), (1, los)):
        st = sc.film_stats_host(*films, 1, mask=m, scale="linear", range=(0.0, 0.0), bins=0)
        assert same_bits(got["min"][zone], st["min"]) and same_bits(got["max"][zone], st["max"]) and np.array_equal(got["n"][zone], st["n"])


# ---- the arithmetic under sanitizers ------------------------------------------------------------------------------------------------------------
def test_exact_sum_under_the_sanitizers(tmp_path):
    """tests/film_zonal_main.cpp, a stand-alone program over fz_add / fz_round, compiled with -fsanitize=undefined,address and run as a child process
    (nothing is preloaded): the shifts are where undefined behaviour would hide."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "film_zonal_main"
    # the sanitizer runtimes are linked statically, so the child needs no runtime library at load time
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "wave_tracer_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "film_zonal_main.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout[-2000:], run.stderr[-2000:])
