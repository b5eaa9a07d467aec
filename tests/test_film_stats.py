"""Film statistics (wt/film_stats.h: wtgpu_film_stats_edges / wtgpu_film_stats_host; imageio.percentiles, render.auto_db_range) on the CPU: the
host twin against a numpy restatement written here (it calls nothing of the library), on synthetic films whose developed values are known
exactly.  tests/test_gpu_film_stats.py runs the device kernels against the host twin on the same films.

What must agree exactly: every counter and every bin (integers; the classification compares f32 values with an f32 edge table, no libm call
per element), min / max / min_positive (bit for bit, -0 below +0) and — the order of additions being fixed — the sum, against a numpy
restatement of that order.  Against math.fsum the sum is held to n 2^-52 sum|x|, the bound of f64 addition in ANY order ((n - 1) roundings of
at most 2^-53 of a partial sum that never exceeds sum|x|, with a factor 2 to spare)."""
import math

import numpy as np
import pytest

from test_sensor_mask import _write
from test_tonemap import F32, MONO, RGB, film_xml, restate_develop

W, H = 37, 23                       # 851 pixels: three whole chunks of 256 and a part of a fourth
LEVELS = (257, 256)                 # W x H = 65,792 pixels: 257 chunk sums, then 2 (the second of ONE sum), then 1 — the smallest film whose chunk sums take two levels
assert [-(-LEVELS[0] * LEVELS[1] // 256), -(-(-(-LEVELS[0] * LEVELS[1] // 256)) // 256)] == [257, 2]
PLANES = {1: (MONO, False, 1, 1), 3: (RGB, False, 3, 1), 4: (MONO, True, 1, 4), 12: (RGB, True, 3, 4)}     # P: response, polarimetric, channels, stokes
BINS = [0, 1, 7, 256, 4096]
RANGES = {"dB": (-50.0, 10.0), "linear": (0.25, 3.0)}
SPE = 7


def stats_scene(d, P, width=W, height=H):
    from wave_tracer_amd import Scene
    resp, pol, channels, stokes = PLANES[P]
    sc = Scene.from_xml(_write(d, f"s{width}_{P}.xml", film_xml(response=resp, width=width, height=height, polarimetric=pol)))
    assert (sc.width, sc.height, sc.spectral_channels, sc.stokes) == (width, height, channels, stokes)
    return sc


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_stats")
    return {P: stats_scene(d, P) for P in PLANES}


# what the two device test files (test_gpu_film_stats.py, test_gpu_film_compare.py) share
def device_scenes(d, sizes):
    """{(W, H, P): uploaded scene}: every plane count at `sizes`, P = 3 and 12 at LEVELS"""
    return {(w, h, P): stats_scene(d, P, w, h).upload(0) for w, h in list(sizes) + [LEVELS] for P in (PLANES if (w, h) != LEVELS else (3, 12))}


def to_device(sc, arrays):
    import torch
    dev = torch.device("cuda", sc.device)
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def restate_edges(scale, lo, hi, bins):
    """lo + i (hi - lo) / bins in f64 (lo and hi as the f32 the spec carries), through 10^(t / 10) for dB, then ONE rounding to f32."""
    lo, hi = float(F32(lo)), float(F32(hi))
    out = []
    for i in range(bins + 1):
        t = lo + i * (hi - lo) / bins if bins else lo
        out.append(F32(math.pow(10.0, t / 10.0) if scale == "dB" else t))
    return np.array(out, dtype=F32)


def key(x):
    """a uint32 that orders the non-NaN f32 as the reals do, -0 below +0"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))


def butterfly_sum(a):
    """The fixed order: chunks of 256 in sequence, a[i] += a[i + d] for d = 128 .. 1, the chunk sums by the same rule; +0.0 where nothing is."""
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return 0.0
    while True:
        pad = (-a.size) % 256
        a = np.concatenate((a, np.zeros(pad))).reshape(-1, 256)
        d = 128
        with np.errstate(all="ignore"):
            while d:
                a = a[:, :d] + a[:, d:2 * d]
                d //= 2
        a = a[:, 0]
        if a.size == 1:
            return float(a[0])


def elements(channels, stokes, films, spe, s, abs_, luminance):
    """[pixels, planes] f32: the developed planes of Stokes component s, the luminance (f32 products added left to right, max(0, .) that sends a
    NaN to 0) behind them, |.| of everything with abs_."""
    d = restate_develop(*films, spe).reshape(-1, channels, stokes)[:, :, s]
    if luminance:
        with np.errstate(all="ignore"):
            lum = (F32(.2126) * d[:, 0] + F32(.7152) * d[:, 1]) + F32(.0722) * d[:, 2]
        d = np.concatenate((d, np.where(0 < lum, lum, F32(0))[:, None]), axis=1)
    return np.abs(d) if abs_ else d


def restate_stats(x, edges, mask):
    """x: [pixels, planes] f32 -> the dict Scene.film_stats_host returns (the statistics only)."""
    bins = len(edges) - 1
    inc = np.ones(len(x), bool) if mask is None else (mask.reshape(-1) > 0)
    out = {k: [] for k in ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above", "min", "max", "min_positive", "sum_butterfly", "fsum", "bound", "hist")}
    for c in range(x.shape[1]):
        v = x[inc, c]
        nan, pos = np.isnan(v), v > 0
        below, above = pos & (v < edges[0]), pos & (v >= edges[-1])
        inbin = pos & ~below & ~above
        idx = np.searchsorted(edges, v[inbin], "right") - 1
        assert bins > 0 or not inbin.any()
        out["hist"].append(np.bincount(idx, minlength=bins).astype(np.uint64) if bins else np.zeros(0, np.uint64))
        for name, sel in (("n", np.ones(len(v), bool)), ("n_nan", nan), ("n_negative", v < 0), ("n_zero", v == 0), ("n_below", below), ("n_above", above)):
            out[name].append(int(sel.sum()))
        real = v[~nan]
        out["min"].append(real[np.argmin(key(real))] if len(real) else F32(np.nan))
        out["max"].append(real[np.argmax(key(real))] if len(real) else F32(np.nan))
        out["min_positive"].append(v[pos].min() if pos.any() else F32(np.nan))
        addends = np.where(inc & ~np.isnan(x[:, c]), x[:, c].astype(np.float64), 0.0)      # excluded and NaN elements add +0.0 in their place
        out["sum_butterfly"].append(butterfly_sum(addends))
        finite = np.isfinite(real).all()
        with np.errstate(all="ignore"):
            out["fsum"].append(math.fsum(float(t) for t in real) if finite else float(np.sum(real.astype(np.float64))))
        out["bound"].append(len(v) * 2.0 ** -52 * math.fsum(abs(float(t)) for t in real) if finite else None)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_against_restatement(got, want, label):
    for name in ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above"):
        assert got[name].dtype == np.uint64 and got[name].tolist() == want[name], (label, name, got[name].tolist(), want[name])
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], np.array(want["hist"], dtype=np.uint64).reshape(got["hist"].shape)), (label, "hist")
    for name in ("min", "max", "min_positive"):
        assert same_bits(got[name], np.array(want[name], dtype=F32)), (label, name, got[name], want[name])
    assert same_bits(got["sum"], np.array(want["sum_butterfly"], dtype=np.float64)), (label, "sum against the restated order", got["sum"], want["sum_butterfly"])
    for c, (s, f, bound) in enumerate(zip(got["sum"], want["fsum"], want["bound"])):
        if bound is None:     # an infinite element: +inf, -inf or (both signs) NaN, whatever the order
            assert (np.isnan(s) and np.isnan(f)) or s == f, (label, c, s, f)
        else:
            assert abs(s - f) <= bound, (label, c, s, f, bound)


# ---- films ------------------------------------------------------------------------------------------------------------------------------------
def ulp_neighbours(e):
    e = F32(e)
    return [np.nextafter(e, F32(-np.inf)), e, np.nextafter(e, F32(np.inf))]


def stats_films(height, width, channels, stokes, seed, edges, infinities=True):
    """Seeded films whose developed values are known f32: weight 1 and no light put `value` itself on the film.  Most pixels: log-uniform positive
    values across and beyond the ranges of RANGES, a fifth negated; every eighth pixel has weight 0 (developed value: light / spe alone, or an
    exact 0).  The first odd pixels hold, in every plane: +0, -0, -1, a NaN, [+inf, -inf,] and edge[0], edge[bins / 2], edge[bins] with the f32
    just below and just above each."""
    rng = np.random.default_rng(seed)
    P, n = channels * stokes, height * width
    x = (10.0 ** rng.uniform(-7.0, 2.0, (n, P))).astype(F32)
    x[rng.random((n, P)) < 0.2] *= F32(-1)
    value, weight = x.astype(np.float64), np.ones(n)
    light = np.zeros((n, P))
    weight[::8] = 0.0
    value[::8] = rng.normal(size=(n, P))[::8]                           # (ignored: the weight is 0)
    light[::8] = (rng.uniform(0.0, 3.0, (n, P)) * (rng.random((n, P)) < 0.5))[::8]
    special = [F32(0.0), F32(-0.0), F32(-1.0), F32(np.nan)] + ([F32(np.inf), F32(-np.inf)] if infinities else [])
    for i in sorted({0, (len(edges) - 1) // 2, len(edges) - 1}):
        special += ulp_neighbours(edges[i])
    assert n >= 2 * len(special) + 2
    for k, e in enumerate(special):
        value[2 * k + 1] = float(e)
    return value.reshape(height, width, P), weight.reshape(height, width), light.reshape(height, width, P)


def checker(height, width):
    yy, xx = np.mgrid[0:height, 0:width]
    m = np.where((yy + xx) % 2 == 0, 0.0, 0.75).astype(F32)
    m.reshape(-1)[[1, 3, 5]] = [np.nan, -1.0, 1e-30]      # a NaN and a negative value exclude, the smallest positive includes
    return m


def option_cases(channels, stokes):
    """(stokes_component, abs, luminance, with mask): all eight combinations of the three switches, the Stokes components in turn"""
    out = []
    for k in range(8):
        abs_, lum, masked = bool(k & 1), bool(k & 2), bool(k & 4)
        if lum and channels != 3:
            continue
        out.append((k % stokes, abs_, lum, masked))
    return out


# ---- errors and edges -----------------------------------------------------------------------------------------------------------------------
def test_refused_specs_say_why(scenes):
    from wave_tracer_amd import WtgpuError
    mono, rgb = scenes[1], scenes[3]
    fm, fr = stats_films(H, W, 1, 1, 1, restate_edges("dB", -50, 10, 4)), stats_films(H, W, 3, 1, 1, restate_edges("dB", -50, 10, 4))
    with pytest.raises(WtgpuError, match=r"stokes_component 1 out of range \(the film has 1\)"):
        mono.film_stats_host(*fm, SPE, stokes_component=1, range=(-50, 10))
    with pytest.raises(WtgpuError, match=r"stokes_component 4 out of range \(the film has 4\)"):
        scenes[12].film_stats_host(*stats_films(H, W, 3, 4, 1, restate_edges("dB", -50, 10, 4)), SPE, stokes_component=4, range=(-50, 10))
    with pytest.raises(WtgpuError, match="bins 4097 above the 4096"):
        rgb.film_stats_host(*fr, SPE, range=(-50, 10), bins=4097)
    for lo, hi in ((10, 10), (10, -50)):
        with pytest.raises(WtgpuError, match="lo < hi expected with bins > 0"):
            rgb.film_stats_host(*fr, SPE, range=(lo, hi), bins=8)
    with pytest.raises(WtgpuError, match="finite range"):
        rgb.film_stats_host(*fr, SPE, range=(-50, float("inf")), bins=8)
    with pytest.raises(WtgpuError, match=r"LUMINANCE needs a 3-channel film \(this one has 1\)"):
        mono.film_stats_host(*fm, SPE, range=(-50, 10), luminance=True)
    # 256 steps between two neighbouring f32, and a dB range whose upper end is beyond f32
    with pytest.raises(WtgpuError, match=r"degenerate edges: edge 1 of 256 is not above edge 0"):
        rgb.film_stats_host(*fr, SPE, scale="linear", range=(1.0, float(np.nextafter(F32(1), F32(2)))), bins=256)
    with pytest.raises(WtgpuError, match="degenerate edges"):
        rgb.film_stats_host(*fr, SPE, scale="dB", range=(0.0, 400.0), bins=4)
    with pytest.raises(ValueError, match="scale"):
        rgb.film_stats_host(*fr, SPE, scale="log")
    with pytest.raises(ValueError, match="films of the scene's size"):
        rgb.film_stats_host(*fm, SPE, range=(-50, 10))
    # bins = 0 asks for no table beyond its one edge: lo >= hi is nobody's business then
    assert rgb.film_stats_host(*fr, SPE, range=(3, 3), bins=0)["hist"].shape == (3, 0)


@pytest.mark.parametrize("scale,lo,hi", [("dB", -50.0, 10.0), ("dB", -123.4, -0.1), ("dB", 0.0, 0.5), ("linear", 0.25, 3.0), ("linear", -1.0, 1e-3), ("linear", 1e-9, 1e9)])
def test_edges_agree_with_the_f64_restatement(built, scale, lo, hi):
    import ctypes as C
    from wave_tracer_amd.api import FILM_STATS_SCALES, FilmStatsSpec, load_library
    for bins in BINS + [3, 1000]:
        spec = FilmStatsSpec(0, FILM_STATS_SCALES.index(scale), bins, 0, lo, hi)
        got = np.full(bins + 2, -7.0, dtype=F32)
        assert load_library().wtgpu_film_stats_edges(C.byref(spec), got.ctypes.data) == 0
        want = restate_edges(scale, lo, hi, bins)
        assert same_bits(got[:-1], want) and got[-1] == -7.0, (scale, lo, hi, bins)
        assert (np.diff(want.astype(np.float64)) > 0).all()


# ---- the host twin against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("P", sorted(PLANES))
def test_host_twin_equals_the_restatement(scenes, P, bins):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    for scale, (lo, hi) in RANGES.items():
        edges = restate_edges(scale, lo, hi, bins)
        for infinities in (False, True):
            films = stats_films(H, W, channels, stokes, 100 + P + bins, edges, infinities)
            for s, abs_, lum, masked in option_cases(channels, stokes):
                m = mask if masked else None
                got = sc.film_stats_host(*films, SPE, stokes_component=s, scale=scale, range=(lo, hi), bins=bins, abs=abs_, luminance=lum, mask=m, threads=3)
                label = (P, bins, scale, infinities, s, abs_, lum, masked)
                assert same_bits(got["edges"], edges) and got["hist"].shape == (channels + lum, bins), label
                want = restate_stats(elements(channels, stokes, films, SPE, s, abs_, lum), edges, m)
                check_against_restatement(got, want, label)
                assert (got["n"] == (H * W if m is None else int((m > 0).sum()))).all()
                if bins and not masked and not lum:     # the film was built to meet every class, and the three edges from both sides
                    assert got["n_nan"].all() and got["n_zero"].all() and got["n_below"].all() and got["n_above"].all() and (abs_ or got["n_negative"].all()), label
                    assert got["hist"][:, 0].all() and got["hist"][:, -1].all(), label


def test_host_twin_equals_the_restatement_over_two_levels(built, tmp_path):
    """At LEVELS the loop over the levels runs twice and its second pass reads what the first wrote; the last chunk of the level above the chunk
    sums holds one sum.  An RGB film with its luminance under the checker mask, every field."""
    w, h = LEVELS
    sc = stats_scene(tmp_path, 3, w, h)
    mask = checker(h, w)
    lo, hi = RANGES["dB"]
    edges = restate_edges("dB", lo, hi, 256)
    for infinities in (False, True):
        films = stats_films(h, w, 3, 1, 700 + infinities, edges, infinities)
        got = sc.film_stats_host(*films, SPE, range=(lo, hi), bins=256, luminance=True, mask=mask, threads=3)
        assert same_bits(got["edges"], edges) and got["hist"].shape == (4, 256) and (got["n"] == int((mask > 0).sum())).all()
        check_against_restatement(got, restate_stats(elements(3, 1, films, SPE, 0, False, True), edges, mask), (LEVELS, infinities))
        assert got["hist"].all(axis=1).any() and got["sum"].all()


def test_the_edge_values_fall_where_the_classes_say(scenes):
    """edge[0] itself is in bin 0 and the f32 below it is below; edge[bins] is above and the f32 below it in the last bin; an inner edge opens
    its own bin.  One pixel each, everything else masked out."""
    sc = scenes[1]
    for scale, (lo, hi) in RANGES.items():
        edges = restate_edges(scale, lo, hi, 7)
        for i, cases in ((0, ("n_below", 0, 0)), (3, (2, 3, 3)), (7, (6, "n_above", "n_above"))):
            for e, where in zip(ulp_neighbours(edges[i]), cases):
                value = np.zeros((H, W, 1))
                value[5, 6] = float(e)
                mask = np.zeros((H, W), F32)
                mask[5, 6] = 1
                got = sc.film_stats_host(value, np.ones((H, W)), np.zeros((H, W, 1)), 0, scale=scale, range=(lo, hi), bins=7, mask=mask)
                assert got["n"][0] == 1 and got["min"][0] == e and got["max"][0] == e and got["min_positive"][0] == e and got["sum"][0] == float(e)
                if isinstance(where, str):
                    assert got[where][0] == 1 and not got["hist"].any(), (scale, i, e, where)
                else:
                    assert got["hist"][0].tolist() == [int(k == where) for k in range(7)], (scale, i, e, where)


def test_nothing_included_gives_nan_extrema(scenes):
    sc = scenes[3]
    films = stats_films(H, W, 3, 1, 5, restate_edges("dB", -50, 10, 7))
    got = sc.film_stats_host(*films, SPE, range=(-50, 10), bins=7, luminance=True, mask=np.zeros((H, W), F32))
    assert not got["n"].any() and not got["hist"].any() and got["hist"].shape == (4, 7) and (got["sum"] == 0).all()
    assert np.isnan(got["min"]).all() and np.isnan(got["max"]).all() and np.isnan(got["min_positive"]).all()


def test_the_result_does_not_depend_on_the_threads(scenes):
    for P in (3, 12):
        _, _, channels, stokes = PLANES[P]
        films = stats_films(H, W, channels, stokes, 9, restate_edges("dB", -50, 10, 256))
        a, b = (scenes[P].film_stats_host(*films, SPE, range=(-50, 10), bins=256, luminance=True, mask=checker(H, W), threads=t) for t in (1, 5))
        assert all(same_bits(a[k], b[k]) for k in ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above", "min", "max", "min_positive", "sum", "hist", "edges"))


def test_range_none_takes_two_passes(scenes):
    """Without a range the first pass finds the smallest positive (dB) or smallest (linear) and the largest element; every element that has a
    place on the axis is then inside the bins."""
    sc = scenes[3]
    films = stats_films(H, W, 3, 1, 4, restate_edges("dB", -50, 10, 4), infinities=False)
    x = elements(3, 1, films, SPE, 0, False, False)
    db = sc.film_stats_host(*films, SPE)
    assert db["bins"] == 256 and db["scale"] == "dB" and not db["n_below"].any() and not db["n_above"].any()
    assert (db["hist"].sum(axis=1) == (x > 0).sum(axis=0)).all()
    lo, hi = 10 * math.log10(float(x[x > 0].min())), 10 * math.log10(float(np.nanmax(x)))
    assert lo - 2e-3 < db["range"][0] < lo and hi < db["range"][1] < hi + 2e-3
    lin = sc.film_stats_host(*films, SPE, scale="linear", abs=True, bins=64)
    assert not lin["n_below"].any() and not lin["n_above"].any() and (lin["hist"].sum(axis=1) == (np.abs(x) > 0).sum(axis=0)).all()
    with pytest.raises(ValueError, match="range=None needs a finite positive element"):
        sc.film_stats_host(np.zeros((H, W, 3)), np.ones((H, W)), np.zeros((H, W, 3)), 1)
    with pytest.raises(ValueError, match="range=None needs a finite"):
        sc.film_stats_host(*stats_films(H, W, 3, 1, 4, restate_edges("dB", -50, 10, 4), infinities=True), SPE)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def test_percentiles_on_hand_made_counts(built):
    from wave_tracer_amd.imageio import percentiles
    u64 = lambda *a: np.array(a, dtype=np.uint64)
    st = {"hist": np.array([[0, 10, 0, 10], [4, 4, 4, 4], [0, 0, 0, 0]], dtype=np.uint64), "range": (0.0, 4.0), "n_below": u64(0, 2, 0), "n_above": u64(0, 2, 0)}
    p = percentiles(st, [0, 25, 50, 75, 100])
    assert p.shape == (3, 5)
    assert p[0].tolist() == [1.0, 1.5, 3.0, 3.5, 4.0]             # ranks 0, 5, 10, 15, 20 of 20: empty bins are stepped over
    assert p[1].tolist() == [0.0, 0.75, 2.0, 3.25, 4.0]           # 2 + 16 + 2: ranks 0 (among those below: lo), 5, 10, 15, 20 (among those above: hi)
    assert np.isnan(p[2]).all()                                   # nothing to rank
    assert percentiles(st, 50).tolist()[:2] == [3.0, 2.0] and percentiles(st, 50).shape == (3,)
    db = {"hist": np.array([[1, 1, 2]], dtype=np.uint64), "range": (-30.0, 0.0), "n_below": u64(0), "n_above": u64(0)}
    assert percentiles(db, [50, 75]).tolist() == [[-10.0, -5.0]]  # in the histogram's own scale
    none = {"hist": np.zeros((1, 0), np.uint64), "range": (-3.0, -3.0), "n_below": u64(3), "n_above": u64(1)}
    assert percentiles(none, [10, 75, 90]).tolist() == [[-3.0, -3.0, -3.0]] and none["range"][0] == none["range"][1]
    with pytest.raises(ValueError):
        percentiles(st, 101)


def test_auto_db_range_on_log_uniform_values(scenes):
    """851 values spread evenly in dB over [-60, 0], shuffled: the 1st and the 99th percentile within one bin width (60.002 / 256 dB) of numpy's."""
    from wave_tracer_amd.render import auto_db_range
    sc = scenes[1]
    db = np.linspace(-60.0, 0.0, H * W)
    x = (10.0 ** (db / 10.0)).astype(F32)
    np.random.default_rng(2).shuffle(x)
    films = (x.astype(np.float64).reshape(H, W, 1), np.ones((H, W)), np.zeros((H, W, 1)))
    width = 60.002 / 256
    for q in ((1, 99), (5, 50)):
        lo, hi = auto_db_range(sc, films, 0, percentiles=q)
        want = np.percentile(10.0 * np.log10(x.astype(np.float64)), q)
        assert abs(lo - want[0]) <= width and abs(hi - want[1]) <= width, (q, lo, hi, want)
    # with a mask only the included pixels count: the upper half of the values
    mask = (x.reshape(H, W) >= F32(1e-3)).astype(F32)
    lo, hi = auto_db_range(sc, films, 0, percentiles=(0, 100), mask=mask)
    inc = 10.0 * np.log10(x[x >= F32(1e-3)].astype(np.float64))
    assert inc.min() < -29.9 and abs(lo - inc.min()) <= 30.1 / 256 and abs(hi - inc.max()) <= 30.1 / 256
    # an RGB film is judged by its luminance
    rgb = (np.repeat(films[0], 3, axis=2) * [1.0, 2.0, 0.5], films[1], np.zeros((H, W, 3)))
    lo3, hi3 = auto_db_range(scenes[3], rgb, 0)
    lum = elements(3, 1, rgb, 0, 0, False, True)[:, 3].astype(np.float64)
    want = np.percentile(10.0 * np.log10(lum), (1, 99))
    assert abs(lo3 - want[0]) <= width and abs(hi3 - want[1]) <= width
