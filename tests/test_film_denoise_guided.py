"""The feature-guided denoiser (wt/film_denoise.h "Guides": wtgpu_film_denoise_guided_host; Scene.film_denoise_host(guide=, guide_scale=, ids=),
render.denoise(guides=), render.first_hit_guides) on the CPU: the host twin against an f64 numpy restatement written here — tests/test_film_denoise.py's
`restate` with the feature distance F, dn_guided and the id condition added —, the consequences of the rule that hold bit for bit, the quality on
films with a disc and a two-pixel bar that are weaker than the noise, every refusal, and the Python layer.  tests/test_gpu_film_denoise_guided.py
holds the device kernels to the host twin on the same films.

Tolerance of the restatement test: 10 x the largest difference measured on these films, relative to the film's largest finite value
(tests/golden/denoise_guided_measured.json; tests/parity.py's convention).  Beside the unguided filter's f32 roundings F adds f32 rounding inside an
exponent: a relative 2^-24 of an F of up to ~35 moves exp(-F) by ~2e-6 of itself — of weights that are below 1e-15 then; near the colour distance
(F ~ D ~ 1) it moves a weight by ~1e-7, which is the size of what the unguided filter already has."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_film_denoise import CASES, KW, PRIMES, SMALL, denoise_films, developed, merged, rel_diff
from test_film_stats import F32, PLANES, SPE, checker, same_bits, stats_scene

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "denoise_guided_measured.json")
MEASURED = json.load(open(GOLDEN))
QUALITY = [((64, 48), 5, 2, 0.1, 0.08), ((64, 48), 3, 1, 0.1, 0.08), ((83, 61), 5, 2, 0.05, 0.04)]        # size, r, f, sigma, c
QUALITY_BAR_BOUND = [0.6, 0.8, 0.6]
GUIDE_SETS = [(1, False), (5, False), (8, False), (0, True), (5, True)]                                   # G, with ids


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_denoise_guided")
    out = {(w, h, P): stats_scene(d, P, w, h) for w, h in (SMALL, PRIMES) for P in PLANES}
    out[(64, 48, 3)] = stats_scene(d, 3, 64, 48)
    return out


# ---- guides -------------------------------------------------------------------------------------------------------------------------------------
def regions(H, W):
    """three regions: left of a slanted line, right of it, and a disc — what a shape map looks like"""
    yy, xx = np.mgrid[0:H, 0:W]
    reg = np.where(xx + 0.3 * yy > 0.55 * W, 1, 0)
    reg[(xx - 0.3 * W) ** 2 + (yy - 0.6 * H) ** 2 < (0.25 * H) ** 2] = 2
    return reg.astype(np.uint32)


def guide_planes(H, W, G, seed):
    """G noise-free planes of O(1): piecewise-constant ones (the region index scaled to 0 .. 1, stripes, seeded levels per region) alternating with
    smooth ones; and their scales, between 0.5 and 8: F stays below ~ 35"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    reg = regions(H, W)
    planes = []
    for g in range(G):
        if g == 0:
            planes.append(0.5 * reg)
        elif g % 2 == 1:
            planes.append(0.5 + 0.5 * np.sin(0.07 * (g + 1) * xx + 0.05 * yy + g))
        elif g % 4 == 2:
            planes.append(((xx // (3 + g)) % 2).astype(np.float64))
        else:
            planes.append(rng.uniform(-1.0, 1.0, 3)[reg])
    guide = np.stack(planes, axis=-1).astype(F32) if G else None
    return guide, (np.linspace(0.5, 8.0, G).astype(F32) if G else None)


# ---- the restatement, f64: test_film_denoise.restate's body plus F, dn_guided and the id condition ----------------------------------------------------
def restate_guided(a, b, stokes, r, f, k, alpha, eps, mask=None, guide=None, scale=None, ids=None):
    """a, b: [H, W, P] developed values; guide [H, W, G] or None, scale [G], ids [H, W] or None.  Returns (out, residual) in f64."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    H, W, P = a.shape
    C_ = P // stokes
    g = np.zeros((H, W, 0)) if guide is None else guide.astype(np.float64).reshape(H, W, -1)
    s = np.zeros(0) if scale is None else np.asarray(scale, dtype=np.float64)
    with np.errstate(all="ignore"):
        ya, yb = a[..., ::stokes], b[..., ::stokes]
        e = 0.5 * (ya - yb) ** 2
        ep = np.pad(e, ((1, 1), (1, 1), (0, 0)), mode="edge")
        v = sum(ep[j:j + H, i:i + W] for j in range(3) for i in range(3)) / 9.0
        ok = np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1)
        if mask is not None:
            ok &= mask > 0
        uy, ux = np.clip(np.arange(-f, H + f), 0, H - 1), np.clip(np.arange(-f, W + f), 0, W - 1)
        filtered, both = [], ok.copy()
        for x, y in ((a, yb), (b, ya)):
            yu, vu = y[uy][:, ux], v[uy][:, ux]
            sw, acc = np.zeros((H, W)), np.zeros((H, W, P))
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    qy, qx = np.clip(np.arange(-f, H + f) + dy, 0, H - 1), np.clip(np.arange(-f, W + f) + dx, 0, W - 1)
                    yq, vq = y[qy][:, qx], v[qy][:, qx]
                    t = (((yu - yq) ** 2 - alpha * (vu + np.minimum(vu, vq))) / (eps + k * k * (vu + vq))).sum(axis=-1)
                    D = sum(t[j:j + H, i:i + W] for j in range(2 * f + 1) for i in range(2 * f + 1)) / (C_ * (2 * f + 1) ** 2)
                    # the candidates: inside the film, valid, in the mask, of the pixel's id
                    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                    yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                    cand = np.zeros((H, W), bool)
                    cand[ys, xs] = ok[yt, xt]
                    if ids is not None:
                        cand[ys, xs] &= ids[yt, xt] == ids[ys, xs]
                    # F(p, q) = sum_g (g_g(p) - g_g(q))^2 s_g, pointwise; the larger of F and D goes into the one exponential
                    gq = np.zeros_like(g)
                    gq[ys, xs] = g[yt, xt]
                    F = (((g - gq) ** 2) * s).sum(axis=-1)
                    Dg = np.where(np.isnan(F), np.nan, np.where(F > D, F, D))
                    w = np.where(np.isnan(Dg), 0.0, np.where(Dg <= 0, 1.0, np.exp(-np.maximum(Dg, 0.0))))
                    w = np.where(cand, w, 0.0)
                    xq = np.zeros_like(x)
                    xq[ys, xs] = x[yt, xt]
                    sw += w
                    acc += np.where(cand[..., None], w[..., None] * (xq - x), 0.0)
            both &= sw > 0
            filtered.append(x + acc / np.where(sw > 0, sw, 1.0)[..., None])
        fa = np.where(both[..., None], filtered[0], a)
        fb = np.where(both[..., None], filtered[1], b)
        return 0.5 * (fa + fb), 0.5 * (fa - fb)


def host_against_restatement(sc, size, P, r, f, masked, G, with_ids, seed):
    W, H = size
    a, b = denoise_films(H, W, P, seed)
    mask = checker(H, W) if masked else None
    guide, scale = guide_planes(H, W, G, seed + 1)
    ids = regions(H, W) if with_ids else None
    got = sc.film_denoise_host(a, SPE, b, SPE, window=r, patch=f, mask=mask, residual=True, threads=0, guide=guide, guide_scale=scale, ids=ids, **KW)
    want, want_res = restate_guided(developed(sc, a), developed(sc, b), sc.stokes, r, f, mask=mask, guide=guide, scale=scale, ids=ids, **KW)
    assert got["film"].dtype == F32 and got["film"].shape == (H, W, sc.spectral_channels, sc.stokes) == got["residual"].shape
    top = np.abs(want).max()
    return rel_diff(got["film"].reshape(H, W, P), want), float(np.abs(got["residual"].reshape(H, W, P) - want_res).max() / top)


def restatement_differences(scenes, P, size, r, f):
    out = []
    for masked in (False, True):
        for G, with_ids in GUIDE_SETS:
            d_film, d_res = host_against_restatement(scenes[size + (P,)], size, P, r, f, masked, G, with_ids, 2000 + P)
            print(f"film_denoise guided host against f64: P {P} {size} r {r} f {f} mask {masked} G {G} ids {with_ids}: film {d_film:.3e} residual {d_res:.3e}")
            out.append(((masked, G, with_ids), d_film, d_res))
    return out


@pytest.mark.parametrize("size,r,f", CASES)
@pytest.mark.parametrize("P", sorted(PLANES))
def test_host_twin_equals_the_restatement(scenes, P, size, r, f):
    """G = 1, 5, 8, ids alone and 5 planes with ids, each with and without the checker mask, film and residual"""
    bound = 10.0 * MEASURED["host_against_f64_restatement"]["max_rel_difference"]
    assert bound < 1e-4, "a difference beyond f32 size is a finding, not a tolerance"
    for what, d_film, d_res in restatement_differences(scenes, P, size, r, f):
        assert d_film <= bound and d_res <= bound, (P, size, r, f, what, d_film, d_res, bound)


# ---- what holds bit for bit ---------------------------------------------------------------------------------------------------------------------------
def _both(sc, a, b, **kw):
    got = sc.film_denoise_host(a, SPE, b, SPE, residual=True, **KW, **kw)
    return got["film"], got["residual"]


def _same(x, y):
    return same_bits(x[0], y[0]) and same_bits(x[1], y[1])


def test_what_changes_no_weight_gives_the_unguided_result(scenes):
    """All scales 0 with finite guides (F = +0: 0 > Dc only where both weights are 1), and SAME_ID with one id everywhere, with and without a mask"""
    for size, P, r, f in ((SMALL, 3, 10, 3), (SMALL, 12, 3, 1), (PRIMES, 4, 5, 2), (SMALL, 1, 4, 0)):
        W, H = size
        sc = scenes[size + (P,)]
        a, b = denoise_films(H, W, P, 21)
        guide, _ = guide_planes(H, W, 5, 22)
        for mask in (None, checker(H, W)):
            plain = _both(sc, a, b, window=r, patch=f, mask=mask)
            assert _same(_both(sc, a, b, window=r, patch=f, mask=mask, guide=guide, guide_scale=0.0), plain), (size, P, "zero scales")
            assert _same(_both(sc, a, b, window=r, patch=f, mask=mask, guide=guide[..., 0], guide_scale=[0.0]), plain), (size, P, "one plane, [H, W]")
            for one in (np.zeros((H, W), np.uint32), np.full((H, W), -1, np.int32)):
                assert _same(_both(sc, a, b, window=r, patch=f, mask=mask, ids=one), plain), (size, P, "one id")
            assert _same(_both(sc, a, b, window=r, patch=f, mask=mask, guide=guide, guide_scale=0.0, ids=np.full((H, W), 7, np.uint32)), plain)
        m, _ = merged(sc, a, b)
        assert (plain[0] != m).mean() > 0.2


def test_a_separating_guide_is_same_id(scenes):
    """The region index as a guide plane with scale 1e6: F >= 1e6 >= 126 / log2 e across regions (weight 0) and +0 inside one — SAME_ID with the
    region index.  And it is not the unguided result."""
    for size, P, r, f in ((SMALL, 3, 10, 3), (PRIMES, 12, 5, 2), (SMALL, 4, 3, 1)):
        W, H = size
        sc = scenes[size + (P,)]
        a, b = denoise_films(H, W, P, 23)
        reg = regions(H, W)
        for mask in (None, checker(H, W)):
            by_guide = _both(sc, a, b, window=r, patch=f, mask=mask, guide=reg.astype(F32), guide_scale=1e6)
            by_id = _both(sc, a, b, window=r, patch=f, mask=mask, ids=reg)
            assert _same(by_guide, by_id), (size, P, mask is not None)
            assert _same(_both(sc, a, b, window=r, patch=f, mask=mask, ids=reg.astype(np.int32)), by_id)
            assert not same_bits(by_id[0], _both(sc, a, b, window=r, patch=f, mask=mask)[0])


def test_the_result_does_not_depend_on_the_threads(scenes):
    W, H = SMALL
    for P in (3, 12):
        sc = scenes[(W, H, P)]
        a, b = denoise_films(H, W, P, 8)
        guide, scale = guide_planes(H, W, 5, 9)
        one, five = (_both(sc, a, b, window=4, patch=1, mask=checker(H, W), threads=n, guide=guide, guide_scale=scale, ids=regions(H, W)) for n in (1, 5))
        assert _same(one, five)


def test_a_constant_film_is_a_fixed_point_with_any_guide(scenes):
    W, H = SMALL
    for P in sorted(PLANES):
        sc = scenes[(W, H, P)]
        const = np.broadcast_to(np.array([0.75, -0.125, 0.3, 0.0, 1e-3, 7.0, -0.0, 2.5, 0.1, 0.2, 0.3, 0.4][:P]).astype(F32).astype(np.float64), (H, W, P))
        films = (np.ascontiguousarray(const), np.ones((H, W)), np.zeros((H, W, P)))
        guide, scale = guide_planes(H, W, 8, 30 + P)
        for r, f in ((10, 3), (3, 1)):
            film, res = _both(sc, films, films, window=r, patch=f, guide=guide, guide_scale=scale, ids=regions(H, W))
            assert same_bits(film.reshape(H, W, P), developed(sc, films)) and np.array_equal(film.reshape(H, W, P), const.astype(F32)), (P, r, f)
            assert not res.any()


def test_window_zero_gives_the_merged_film(scenes):
    for size in (SMALL, PRIMES):
        W, H = size
        for P in sorted(PLANES):
            sc = scenes[size + (P,)]
            a, b = denoise_films(H, W, P, 7)
            guide, scale = guide_planes(H, W, 5, 8)
            for f in (0, 2):
                assert _same(_both(sc, a, b, window=0, patch=f, guide=guide, guide_scale=scale, ids=regions(H, W)), merged(sc, a, b)), (size, P, f)


BAD_GUIDE = [((12, 10), 1, np.nan), ((5, 25), 0, np.inf), ((20, 30), 4, -np.inf)]       # (row, column), plane, value


def guide_with_bad_pixels(H, W, G, seed):
    guide, scale = guide_planes(H, W, G, seed)
    for (y, x), plane, val in BAD_GUIDE:
        guide[y, x, plane % G] = val
    return guide, scale


def check_bad_guide(sc, a, b, guide, scale, both, **kw):
    """`both(sc, a, b, **kw) -> (film, residual)` with the non-finite guide: exactly those pixels pass through, and they are nobody's candidate — the
    whole result is the one with a finite guide and those pixels masked out."""
    H, W = guide.shape[:2]
    m, d = merged(sc, a, b)
    film, res = both(sc, a, b, guide=guide, guide_scale=scale, **kw)
    clean, mask = guide.copy(), np.ones((H, W), F32)
    for (y, x), _, _ in BAD_GUIDE:
        assert same_bits(film[y, x], m[y, x]) and same_bits(res[y, x], d[y, x])
        clean[y, x], mask[y, x] = 0.0, 0.0
    masked = both(sc, a, b, guide=clean, guide_scale=scale, mask=mask, **kw)
    assert _same((film, res), masked)
    assert np.isfinite(film).all() and np.isfinite(res).all() and (film != m).mean() > 0.3


def test_non_finite_guides_pass_through_and_are_nobodys_candidate(scenes):
    W, H = SMALL
    for P in (3, 12):
        sc = scenes[(W, H, P)]
        a, b = denoise_films(H, W, P, 11)
        for G, zero in ((5, False), (8, False), (5, True)):
            guide, scale = guide_with_bad_pixels(H, W, G, 12)
            scale = scale * 0 if zero else scale                    # (inf x 0 is a NaN: weight 0 all the same)
            for r, f in ((3, 1), (6, 3)):
                check_bad_guide(sc, a, b, guide, scale, _both, window=r, patch=f)
    # exactly that pixel: a film without outliers, where every other pixel finds candidates and is changed
    sc = scenes[(W, H, 3)]
    rng = np.random.default_rng(13)
    a, b = ((( 0.5 + 0.05 * rng.normal(size=(H, W, 3))).astype(F32).astype(np.float64), np.ones((H, W)), np.zeros((H, W, 3))) for _ in range(2))
    guide, scale = guide_with_bad_pixels(H, W, 5, 14)
    film, res = _both(sc, a, b, window=3, patch=1, guide=guide, guide_scale=scale)
    m, d = merged(sc, a, b)
    passed = (film.view(np.uint32) == m.view(np.uint32)).all(axis=(-1, -2))
    want = np.zeros((H, W), bool)
    for (y, x), _, _ in BAD_GUIDE:
        want[y, x] = True
    assert np.array_equal(passed, want)


def test_a_mask_that_excludes_everything(scenes):
    W, H = SMALL
    for P in (1, 12):
        sc = scenes[(W, H, P)]
        a, b = denoise_films(H, W, P, 9)
        nothing = np.zeros((H, W), F32)
        nothing[0, 0], nothing[0, 1] = np.nan, -1.0
        guide, scale = guide_planes(H, W, 5, 10)
        assert _same(_both(sc, a, b, window=3, patch=1, mask=nothing, guide=guide, guide_scale=scale, ids=regions(H, W)), merged(sc, a, b))


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------------
def quality_films(size, sigma, c):
    """shape map 0, a disc (1) and a two-pixel bar (2); truth 0.5, 0.5 + c, 0.5 - c by shape in three channels plus a ramp of 0 .. 0.1 down channel 1;
    two halves with independent N(0, sigma) noise"""
    W, H = size
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    shape = np.zeros((H, W), np.uint32)
    shape[(xx - 0.3 * W) ** 2 + (yy - 0.5 * H) ** 2 < (0.3 * H) ** 2] = 1
    shape[:, int(0.75 * W):int(0.75 * W) + 2] = 2
    truth = np.repeat(np.array([0.5, 0.5 + c, 0.5 - c])[shape][..., None], 3, axis=-1)
    truth[..., 1] += np.linspace(0.0, 0.1, H)[:, None]
    halves = [((truth + sigma * rng.normal(size=truth.shape)).astype(F32).astype(np.float64), np.ones((H, W)), np.zeros((H, W, 3))) for _ in range(2)]
    return truth, shape, halves


def quality_figures(sc, size, r, f, sigma, c):
    W, H = size
    truth, shape, (a, b) = quality_films(size, sigma, c)
    guide = np.stack([shape == 1, shape == 2], axis=-1).astype(F32)
    rms = lambda t: float(np.sqrt((t ** 2).mean()))
    out = {}
    for name, kw in (("unguided", {}), ("guided", dict(guide=guide, guide_scale=8.0)), ("same_id", dict(ids=shape))):
        got = sc.film_denoise_host(a, 1, b, 1, window=r, patch=f, residual=True, **KW, **kw)
        film, res = got["film"].reshape(H, W, 3).astype(np.float64), got["residual"].reshape(H, W, 3).astype(np.float64)
        out[name] = {"whole": rms(film - truth), "bar": rms((film - truth)[shape == 2]), "residual_rms": rms(res)}
    out["merged"] = {"whole": rms(0.5 * (a[0] + b[0]) - truth), "bar": rms((0.5 * (a[0] + b[0]) - truth)[shape == 2])}
    return out


@pytest.mark.parametrize("case", range(len(QUALITY)))
def test_quality_on_a_disc_and_a_bar_weaker_than_the_noise(scenes, case):
    """The yardstick is the existing unguided call on the same films.  Figures of the f64 restatement (whole film unguided / guided, bar unguided /
    guided): 0.0167 / 0.0100, 0.0562 / 0.0225;  0.0186 / 0.0156, 0.0450 / 0.0291;  0.0077 / 0.0047, 0.0302 / 0.0081.  The twin's own figures are printed
    and stand in tests/golden/denoise_guided_measured.json."""
    size, r, f, sigma, c = QUALITY[case]
    q = quality_figures(scenes[size + (3,)], size, r, f, sigma, c)
    u, g, s = q["unguided"], q["guided"], q["same_id"]
    print(f"film_denoise guided quality {size} r {r} f {f} sigma {sigma} c {c}: whole unguided {u['whole']:.4f} guided {g['whole']:.4f} same_id {s['whole']:.4f} "
          f"merged {q['merged']['whole']:.4f}; bar unguided {u['bar']:.4f} guided {g['bar']:.4f} same_id {s['bar']:.4f} merged {q['merged']['bar']:.4f}; "
          f"residual rms / rmse guided {g['residual_rms'] / g['whole']:.3f} same_id {s['residual_rms'] / s['whole']:.3f}")
    assert g["bar"] <= QUALITY_BAR_BOUND[case] * u["bar"]
    assert g["whole"] <= 0.9 * u["whole"]
    assert abs(s["whole"] / g["whole"] - 1.0) <= 0.02 and abs(s["bar"] / g["bar"] - 1.0) <= 0.02
    assert 0.5 <= g["residual_rms"] / g["whole"] <= 2.0 and 0.5 <= s["residual_rms"] / s["whole"] <= 2.0


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_say_why(scenes):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmDenoiseGuides, FilmDenoiseSpec, load_library
    W, H = SMALL
    sc = scenes[(W, H, 3)]
    a, b = denoise_films(H, W, 3, 1)
    guide, scale = guide_planes(H, W, 5, 2)
    ids = regions(H, W)
    call = lambda **kw: sc.film_denoise_host(a, SPE, b, SPE, **kw)
    with pytest.raises(WtgpuError, match=r"n_guides 9 out of range \(0 \.\. 8\)"):
        call(guide=np.zeros((H, W, 9), F32))
    for s in (-1.0, float("nan"), float("inf"), -0.5):
        with pytest.raises(WtgpuError, match="scale 0: a finite value >= 0 expected"):
            call(guide=guide, guide_scale=s)
    with pytest.raises(WtgpuError, match="scale 3: a finite value >= 0 expected"):
        call(guide=guide, guide_scale=[1, 1, 1, -1e-3, 1])
    # everything the unguided call refuses, with the same messages
    with pytest.raises(WtgpuError, match=r"window_radius 11 out of range \(0 \.\. 10\)"):
        call(window=11, guide=guide)
    with pytest.raises(WtgpuError, match=r"patch_radius 4 out of range \(0 \.\. 3\)"):
        call(patch=4, ids=ids)
    with pytest.raises(WtgpuError, match="a finite k > 0 expected"):
        call(k=0.0, guide=guide)
    with pytest.raises(WtgpuError, match="a finite alpha >= 0 expected"):
        call(alpha=-0.5, guide=guide)
    with pytest.raises(WtgpuError, match="a finite eps > 0 expected"):
        call(eps=0.0, ids=ids)
    # what the Python method says itself
    with pytest.raises(ValueError, match=r"guide: \[H, W\] or \[H, W, G\] f32 of the scene's size"):
        call(guide=np.zeros((H, W + 1, 2), F32))
    with pytest.raises(ValueError, match=r"guide: \[H, W\] or \[H, W, G\] f32 of the scene's size"):
        call(guide=np.zeros((H * W * 2,), F32))
    with pytest.raises(ValueError, match="guide_scale: a scalar or 5 values expected, got 3"):
        call(guide=guide, guide_scale=[1, 2, 3])
    with pytest.raises(ValueError, match="guide_scale without a guide"):
        call(guide_scale=2.0)
    with pytest.raises(ValueError, match="ids: .* int32 or uint32 of the scene's size"):
        call(ids=ids.astype(np.int64))
    with pytest.raises(ValueError, match="ids: .* int32 or uint32 of the scene's size"):
        call(ids=ids[:, :-1])
    with pytest.raises(ValueError, match="films of the scene's size"):
        scenes[(W, H, 1)].film_denoise_host(a, SPE, b, SPE, guide=guide)
    with pytest.raises(ValueError, match="a mask of the scene's size"):
        call(guide=guide, mask=np.ones((H, W + 1), F32))
    assert call(window=1, patch=0, guide=guide, guide_scale=scale, ids=ids)["residual"] is None
    # what the Python method cannot say goes to the entry point itself
    lib = load_library()
    ptrs = [np.ascontiguousarray(t).ctypes.data for t in a + b]
    out = np.zeros((H, W, 3), F32)
    spec = FilmDenoiseSpec(1, 1, 0, 0, 0.45, 1.0, 1e-10, 0.0)

    def host(n, flags, g, i, spec=spec, out=out, guides=True):
        gs = FilmDenoiseGuides(n, flags)
        for j in range(8):
            gs.scale[j] = 1.0
        rc = lib.wtgpu_film_denoise_guided_host(sc.handle, *ptrs[:3], SPE, *ptrs[3:], SPE, C.byref(spec), C.byref(gs) if guides else None,
                                                None if g is None else g.ctypes.data, None if i is None else i.ctypes.data, None, 1,
                                                None if out is None else out.ctypes.data, None)
        return rc, lib.wtgpu_last_error()

    for args, message in (((9, 0, guide, None), b"n_guides 9 out of range"), ((5, 2, guide, None), b"unknown flag bits"), ((5, 0x80000001, guide, ids), b"unknown flag bits"),
                          ((5, 0, None, None), b"n_guides > 0 without a guide buffer"), ((0, 1, None, None), b"SAME_ID without an id plane"),
                          ((5, 1, guide, None), b"SAME_ID without an id plane"), ((0, 1, guide, ids), b"a guide buffer with n_guides = 0"),
                          ((5, 0, guide, ids), b"an id plane without SAME_ID"), ((0, 0, None, None), b"neither guides nor SAME_ID")):
        rc, said = host(*args)
        assert rc == 1 and message in said, (args[:2], said)
    assert host(5, 1, guide, ids, out=None) == (1, b"null argument") and host(5, 1, guide, ids, guides=False) == (1, b"null argument")
    rc, said = host(5, 1, guide, ids, spec=FilmDenoiseSpec(1, 1, 4, 0, 0.45, 1.0, 1e-10, 0.0))
    assert rc == 1 and b"no flags are defined" in said                      # SAME_ID is a flag of the guides, not of the spec
    assert host(5, 1, guide, ids)[0] == 0 and out.any()
    # ... and the unguided entry point still refuses every flag
    assert lib.wtgpu_film_denoise_host(sc.handle, *ptrs[:3], SPE, *ptrs[3:], SPE, C.byref(FilmDenoiseSpec(1, 1, 1, 0, 0.45, 1.0, 1e-10, 0.0)), None, 1,
                                       out.ctypes.data, None) == 1
    assert b"no flags are defined" in lib.wtgpu_last_error()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------------
def test_render_denoise_with_guides_on_numpy_films(scenes):
    from wave_tracer_amd.render import denoise
    W, H = SMALL
    sc = scenes[(W, H, 12)]
    a, b = denoise_films(H, W, 12, 12)
    guide, scale = guide_planes(H, W, 5, 13)
    ids = regions(H, W)
    want = sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, residual=True, guide=guide, guide_scale=scale, ids=ids)
    got = denoise(sc, a, b, SPE, guides=(guide, scale, ids), window=3, patch=1)
    assert same_bits(got["film"], want["film"]) and same_bits(got["residual"], want["residual"]) and 0 < got["residual_rel"] < 0.2
    plain = sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, residual=True)
    assert not same_bits(want["film"], plain["film"])
    for none in (None, False):                                              # the default is the unguided call
        got = denoise(sc, a, b, SPE, guides=none, window=3, patch=1)
        assert same_bits(got["film"], plain["film"]) and same_bits(got["residual"], plain["residual"])
    only_ids = denoise(sc, a, b, SPE, guides=(None, None, ids), window=3, patch=1)
    assert same_bits(only_ids["film"], sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, ids=ids)["film"])
    only_guide = denoise(sc, a, b, SPE, guides=(guide, 2.0, None), window=3, patch=1, residual=False)
    assert only_guide["residual"] is None and same_bits(only_guide["film"], sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, guide=guide, guide_scale=2.0)["film"])


def test_first_hit_guides(built, tmp_path):
    """On the analytic scene of the mask's tests (a camera above two rectangles, sky beyond), through first_hit_host: shape, dtype, the planes, zeros where
    nothing is hit; denoise(guides=True) takes them; the refusal on a virtual-plane sensor is first_hit's own."""
    from test_sensor_mask import MASK, _write, analytic_xml, masked_radio_xml
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.render import FIRST_HIT_GUIDE_KF, denoise, first_hit_guides
    sc = Scene.from_xml(_write(tmp_path, "ab.xml", analytic_xml()))
    H, W = sc.height, sc.width
    guide, scales, ids = first_hit_guides(sc, host=True)
    fh = sc.first_hit_host(samples=0, maps=("coverage", "depth", "normal_shading"), ids=("shape",))
    assert guide.shape == (H, W, 5) and guide.dtype == F32 and guide.flags["C_CONTIGUOUS"] and ids.shape == (H, W) and ids.dtype == np.uint32
    assert scales == [1.0 / FIRST_HIT_GUIDE_KF ** 2] * 5 and scales[0] == pytest.approx(2.7778, rel=1e-4)
    hit = fh["coverage"] > 0
    assert hit.any() and not hit.all() and np.isfinite(guide).all()
    assert same_bits(guide[..., :3], fh["normal_shading"]) and same_bits(guide[..., 4], fh["coverage"]) and same_bits(ids, fh["shape"])
    assert np.array_equal(guide[..., 3][hit], np.log(fh["depth"][hit])) and not guide[~hit].any() and (ids[~hit] == 0xFFFFFFFF).all() and (ids[hit] != 0xFFFFFFFF).all()
    g7, s7, none = first_hit_guides(sc, samples=7, seed=3, scales=[1, 2, 3, 4, 5], same_shape=False, host=True)
    assert none is None and s7 == [1.0, 2.0, 3.0, 4.0, 5.0] and g7.shape == (H, W, 5) and ((g7[..., 4] > 0) & (g7[..., 4] < 1)).any()
    assert first_hit_guides(sc, scales=4.0, host=True)[1] == [4.0] * 5
    assert (sc.spectral_channels, sc.stokes) == (3, 1)
    rng = np.random.default_rng(5)
    a, b = (((0.5 + 0.05 * rng.normal(size=(H, W, 3))).astype(F32).astype(np.float64), np.ones((H, W)), np.zeros((H, W, 3))) for _ in range(2))
    got = denoise(sc, a, b, 1, guides=True, window=3, patch=1)                # (numpy films: the guides come from first_hit_host)
    want = sc.film_denoise_host(a, 1, b, 1, window=3, patch=1, residual=True, guide=guide, guide_scale=scales, ids=ids)
    assert same_bits(got["film"], want["film"]) and same_bits(got["residual"], want["residual"])
    assert not same_bits(got["film"], sc.film_denoise_host(a, 1, b, 1, window=3, patch=1)["film"])
    vp = Scene.from_xml(_write(tmp_path, "vp.xml", masked_radio_xml(MASK, "virtual_plane")), defines={}, res=32)
    with pytest.raises(WtgpuError, match="perspective sensor"):
        first_hit_guides(vp, host=True)
    with pytest.raises(WtgpuError, match="upload"):
        first_hit_guides(sc)
