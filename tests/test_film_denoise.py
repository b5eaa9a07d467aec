"""The denoiser of two half-films (wt/film_denoise.h: wtgpu_film_denoise_host; render.denoise, render_to_noise(halves=True)) on the CPU: the host twin
against an f64 numpy restatement written here (it calls nothing of the library but wtgpu_develop, whose f32 values are the filter's inputs by
definition; np.exp for the weight; vectorised per window offset), the bound of dn_exp2_neg, the properties that hold bit for bit, and the quality
on three synthetic films.  tests/test_gpu_film_denoise.py runs the device kernels against the host twin on the same films.

Tolerance of the restatement test: 10 x the largest difference measured on these films, relative to the film's largest finite value
(tests/golden/denoise_measured.json; tests/parity.py's convention).  The measured differences are of f32 size: the twin rounds every operation to
f32, the restatement none.  The refusal of a film whose channel count is not 1 or 3 cannot be reached from here: no sensor response builds one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_film_stats import F32, PLANES, SPE, checker, same_bits, stats_scene

MEASURED = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "denoise_measured.json")))
SMALL, PRIMES = (37, 23), (83, 61)              # W x H; 83 x 61: six by four 16 x 16 tiles of the device kernel, the last of each row and column partial
CASES = [(SMALL, 10, 3), (SMALL, 3, 1), (PRIMES, 5, 2)]
QUALITY = [((64, 48), 5, 2, 0.1), ((64, 48), 3, 1, 0.1), ((83, 61), 5, 2, 0.05)]
KW = dict(k=0.45, alpha=1.0, eps=1e-10)


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_denoise")
    out = {(w, h, P): stats_scene(d, P, w, h) for w, h in (SMALL, PRIMES) for P in PLANES}
    out[(64, 48, 3)] = stats_scene(d, 3, 64, 48)
    return out


# ---- films ------------------------------------------------------------------------------------------------------------------------------------
def denoise_films(height, width, P, seed, sigma=0.05):
    """Two half-film sets of one seeded scene: a smooth pattern with an edge per plane (the signed Stokes planes smaller), independent Gaussian noise
    in each half, all values exact f32 at weight 1 without light; every 29th pixel has weight 0 in both halves (developed value: light / spe alone —
    the pattern again, but for every other of them, an exact 0 that stands out of its neighbourhood) and the first pixels hold +0, -0 and a negative
    value.  Few outliers: a patch that holds one matches nothing, and a film full of them would leave the filter nothing to do."""
    _, _, channels, stokes = PLANES[P]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    truth = np.zeros((height, width, P))
    for i in range(P):
        s = i % stokes
        base = 0.5 + 0.3 * np.sin(0.05 * xx + 0.03 * (i + 1) * yy) + np.where(xx > width * (0.3 + 0.04 * i), 0.4, 0.0)
        truth[..., i] = base if s == 0 else 0.2 * (base - 0.7)
    sets = []
    for _ in range(2):
        value = (truth + sigma * rng.normal(size=truth.shape)).astype(F32).astype(np.float64)
        value.reshape(-1, P)[0], value.reshape(-1, P)[1], value.reshape(-1, P)[2] = 0.0, -0.0, -0.25
        weight, light = np.ones((height, width)), np.zeros((height, width, P))
        weight.reshape(-1)[::29] = 0.0
        light.reshape(-1, P)[29::58] = (SPE * value.reshape(-1, P)[29::58]).astype(F32)
        sets.append((value, weight, light))
    return sets


def developed(sc, films, spe=SPE):
    from wave_tracer_amd.render import develop
    return develop(sc, *films, spe).reshape(sc.height, sc.width, -1)


def merged(sc, a, b):
    """(a + b) x 0.5f and (a - b) x 0.5f in f32, a NaN as the quiet NaN: what a pass-through pixel gets"""
    da, db = developed(sc, a), developed(sc, b)
    with np.errstate(invalid="ignore", over="ignore"):
        m, d = (da + db) * F32(0.5), (da - db) * F32(0.5)
    for t in (m, d):
        t.view(np.uint32)[np.isnan(t)] = 0x7fc00000
    shape = (sc.height, sc.width, sc.spectral_channels, sc.stokes)
    return m.reshape(shape), d.reshape(shape)


# ---- the restatement, f64 ---------------------------------------------------------------------------------------------------------------------------
def restate(a, b, stokes, r, f, k, alpha, eps, mask=None):
    """a, b: [H, W, P] developed values.  Returns (out, residual) in f64, NaN where the twin stores one."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    H, W, P = a.shape
    C_ = P // stokes
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
                    s = (((yu - yq) ** 2 - alpha * (vu + np.minimum(vu, vq))) / (eps + k * k * (vu + vq))).sum(axis=-1)
                    D = sum(s[j:j + H, i:i + W] for j in range(2 * f + 1) for i in range(2 * f + 1)) / (C_ * (2 * f + 1) ** 2)
                    w = np.where(np.isnan(D), 0.0, np.where(D <= 0, 1.0, np.exp(-np.maximum(D, 0.0))))
                    # the candidates: inside the film, valid, in the mask
                    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                    yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                    cand = np.zeros((H, W), bool)
                    cand[ys, xs] = ok[yt, xt]
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


def rel_diff(got, want):
    """largest |got - want| over the elements finite in `want`, relative to the largest finite |want|; the non-finite elements must be the same"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    return float(np.abs(got[fin].astype(np.float64) - want[fin]).max() / np.abs(want[fin]).max())


def host_against_restatement(sc, size, P, r, f, masked, seed):
    W, H = size
    a, b = denoise_films(H, W, P, seed)
    mask = checker(H, W) if masked else None
    got = sc.film_denoise_host(a, SPE, b, SPE, window=r, patch=f, mask=mask, residual=True, threads=0, **KW)
    want, want_res = restate(developed(sc, a), developed(sc, b), sc.stokes, r, f, mask=mask, **KW)
    assert got["film"].dtype == F32 and got["film"].shape == (H, W, sc.spectral_channels, sc.stokes) == got["residual"].shape
    scale = np.abs(want).max()
    return rel_diff(got["film"].reshape(H, W, P), want), float(np.abs(got["residual"].reshape(H, W, P) - want_res).max() / scale)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size,r,f", CASES)
@pytest.mark.parametrize("P", sorted(PLANES))
def test_host_twin_equals_the_restatement(scenes, P, size, r, f, masked):
    d_film, d_res = host_against_restatement(scenes[size + (P,)], size, P, r, f, masked, 1000 + P)
    print(f"film_denoise host against f64: P {P} {size} r {r} f {f} mask {masked}: film {d_film:.3e} residual {d_res:.3e}")
    bound = 10.0 * MEASURED["host_against_f64_restatement"]["max_rel_difference"]
    assert bound < 1e-4, "a difference beyond f32 size is a finding, not a tolerance"
    assert d_film <= bound and d_res <= bound, (P, size, r, f, masked, d_film, d_res, bound)


# ---- dn_exp2_neg --------------------------------------------------------------------------------------------------------------------------------
def exp2_neg_sweep():
    rng = np.random.default_rng(3)
    t = np.concatenate([np.linspace(0.0, 200.0, 200001), rng.uniform(0.0, 126.0, 100000), np.arange(0.0, 201.0), np.arange(0.0, 127.0) + 0.5,
                        np.nextafter(np.arange(1.0, 128.0).astype(F32), F32(0)), [125.99999, 126.0, 126.00001, 1e30, np.inf]]).astype(F32)
    return t


def test_exp2_neg_is_within_its_bound():
    """Relative error <= 1e-6 against f64 exp2 where t < 126 — the result is above 2^-126 — and exactly 0 from t = 126 on, where it would be 2^-126 or
    less (wt/film_denoise.h).  A NaN gives 0, and 2^-0 is exactly 1."""
    from wave_tracer_amd.api import dn_exp2_neg
    t = exp2_neg_sweep()
    got = dn_exp2_neg(t).astype(np.float64)
    small = t < 126.0
    want = np.exp2(-t[small].astype(np.float64))
    err = float(np.abs(got[small] / want - 1.0).max())
    print(f"dn_exp2_neg: largest relative error over {small.sum()} arguments {err:.3e}")
    assert err <= 1e-6 and (got[~small] == 0.0).all() and (~small).sum() > 70000
    assert err <= 10.0 * MEASURED["dn_exp2_neg"]["max_rel_error"]
    assert dn_exp2_neg(np.array([np.nan], F32))[0] == 0.0 and dn_exp2_neg(np.array([0.0], F32))[0] == 1.0
    assert (np.diff(dn_exp2_neg(np.linspace(0, 126, 4001).astype(F32))) <= 0).all()       # (monotone on a grid that crosses every integer)


# ---- exact properties ---------------------------------------------------------------------------------------------------------------------------
def test_a_constant_film_is_a_fixed_point(scenes):
    W, H = SMALL
    for P in sorted(PLANES):
        sc = scenes[(W, H, P)]
        const = np.broadcast_to(np.array([0.75, -0.125, 0.3, 0.0, 1e-3, 7.0, -0.0, 2.5, 0.1, 0.2, 0.3, 0.4][:P]).astype(F32).astype(np.float64), (H, W, P))
        films = (np.ascontiguousarray(const), np.ones((H, W)), np.zeros((H, W, P)))
        for r, f in ((10, 3), (3, 1)):
            got = sc.film_denoise_host(films, SPE, films, SPE, window=r, patch=f, residual=True, **KW)
            assert same_bits(got["film"].reshape(H, W, P), developed(sc, films)) and np.array_equal(got["film"].reshape(H, W, P), const.astype(F32)), (P, r, f)
            assert not got["residual"].any()


def test_window_zero_gives_the_merged_film(scenes):
    for size in (SMALL, PRIMES):
        for P in sorted(PLANES):
            sc = scenes[size + (P,)]
            a, b = denoise_films(size[1], size[0], P, 7)
            m, d = merged(sc, a, b)
            for f in (0, 2):
                got = sc.film_denoise_host(a, SPE, b, SPE, window=0, patch=f, residual=True, **KW)
                assert same_bits(got["film"], m) and same_bits(got["residual"], d), (size, P, f)


def test_the_result_does_not_depend_on_the_threads(scenes):
    W, H = SMALL
    for P in (3, 12):
        sc = scenes[(W, H, P)]
        a, b = denoise_films(H, W, P, 8)
        one, five = (sc.film_denoise_host(a, SPE, b, SPE, window=4, patch=1, mask=checker(H, W), residual=True, threads=n, **KW) for n in (1, 5))
        assert same_bits(one["film"], five["film"]) and same_bits(one["residual"], five["residual"])


def test_masked_out_pixels_are_the_merged_film(scenes):
    W, H = SMALL
    for P in (1, 12):
        sc = scenes[(W, H, P)]
        a, b = denoise_films(H, W, P, 9)
        m, d = merged(sc, a, b)
        nothing = np.zeros((H, W), F32)
        nothing[0, 0], nothing[0, 1] = np.nan, -1.0
        got = sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, mask=nothing, residual=True, **KW)
        assert same_bits(got["film"], m) and same_bits(got["residual"], d)
        mask = checker(H, W)
        got = sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, mask=mask, residual=True, **KW)
        out = ~(mask > 0)
        assert same_bits(got["film"][out], m[out]) and same_bits(got["residual"][out], d[out])
        assert (got["film"][mask > 0] != m[mask > 0]).mean() > 0.5          # ... and most of the others are changed by the filter


def test_one_set_of_weights_serves_all_planes(scenes):
    """A plane that is exactly half another in both halves comes out as half the other: scaling by a power of two is exact as long as nothing
    underflows, so this holds bit for bit only if both planes saw the same weights and the same order of additions.  The films are flat but for
    their noise and k is large, so that no weight comes near 2^-126 (a product of such a weight is a subnormal number, whose half is rounded)."""
    W, H = SMALL
    for P, (src, dst) in ((4, (0, 2)), (12, (5, 9)), (3, (0, 2))):
        sc = scenes[(W, H, P)]
        rng = np.random.default_rng(10 + P)
        halves = []
        for _ in range(2):
            value = (0.5 + 0.1 * np.arange(P) + 0.05 * rng.normal(size=(H, W, P))).astype(F32).astype(np.float64)
            light = (0.01 * SPE * rng.random((H, W, P))).astype(F32).astype(np.float64)
            value[..., dst], light[..., dst] = 0.5 * value[..., src], 0.5 * light[..., src]
            halves.append((value, np.ones((H, W)), light))
        got = sc.film_denoise_host(halves[0], SPE, halves[1], SPE, window=5, patch=2, residual=True, k=1.5, alpha=1.0, eps=1e-10)
        m, _ = merged(sc, *halves)
        for t in (got["film"].reshape(H, W, P), got["residual"].reshape(H, W, P)):
            assert same_bits(t[..., dst], F32(0.5) * t[..., src]) and np.abs(t[t != 0]).min() > 1e-30, P
        assert got["residual"].any() and (got["film"] != m).mean() > 0.9


BAD = [((12, 10), 1, 0, np.nan), ((5, 25), 2, 1, np.inf), ((20, 30), 0, 0, -np.inf)]       # (row, column), plane, half, value


def films_with_bad_pixels(H, W, P, seed):
    a, b = denoise_films(H, W, P, seed)
    for (y, x), plane, half, val in BAD:
        (a, b)[half][0][y, x, plane % P] = val
        (a, b)[half][1][y, x] = 1.0
    return a, b


def check_bad_pixels(film, residual, m, d, f):
    """film, residual, m (merged), d: [H, W, P]"""
    H, W, P = film.shape
    far = np.ones((H, W), bool)
    want_bad = np.zeros((H, W, P), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for (y, x), plane, _, val in BAD:
        want_bad[y, x, plane % P] = True
        far &= np.maximum(abs(yy - y), abs(xx - x)) > f + 1
        assert same_bits(film[y, x], m[y, x]) and same_bits(residual[y, x], d[y, x])          # passes through
        if np.isnan(val):
            assert film[y, x, plane % P].view(np.uint32) == 0x7fc00000 == residual[y, x, plane % P].view(np.uint32)
    assert np.array_equal(~np.isfinite(film), want_bad) and np.array_equal(~np.isfinite(residual), want_bad)
    assert np.isfinite(film[far]).all() and (film[far] != m[far]).mean() > 0.3                 # ... and away from them the filter works


def test_non_finite_pixels_pass_through_and_stay_alone(scenes):
    W, H = SMALL
    for P in (3, 12):
        sc = scenes[(W, H, P)]
        a, b = films_with_bad_pixels(H, W, P, 11)
        m, d = merged(sc, a, b)
        for r, f in ((3, 1), (6, 3)):
            got = sc.film_denoise_host(a, SPE, b, SPE, window=r, patch=f, residual=True, **KW)
            check_bad_pixels(got["film"].reshape(H, W, P), got["residual"].reshape(H, W, P), m.reshape(H, W, P), d.reshape(H, W, P), f)


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------
def quality_films(size, sigma):
    """truth: a two-level step 0.2 / 0.8 with a ramp of 0 .. 0.2 down one channel; two halves with independent N(0, sigma) noise"""
    W, H = size
    rng = np.random.default_rng(7)
    truth = np.empty((H, W, 3))
    truth[:, : W // 2], truth[:, W // 2:] = 0.2, 0.8
    truth[..., 1] += np.linspace(0.0, 0.2, H)[:, None]
    halves = [((truth + sigma * rng.normal(size=truth.shape)).astype(F32).astype(np.float64), np.ones((H, W)), np.zeros((H, W, 3))) for _ in range(2)]
    return truth, halves


@pytest.mark.parametrize("size,r,f,sigma", QUALITY)
def test_quality_on_a_step_with_a_ramp(scenes, size, r, f, sigma):
    W, H = size
    sc = scenes[(W, H, 3)]
    truth, (a, b) = quality_films(size, sigma)
    got = sc.film_denoise_host(a, 1, b, 1, window=r, patch=f, residual=True, **KW)
    film, res = got["film"].reshape(H, W, 3).astype(np.float64), got["residual"].reshape(H, W, 3).astype(np.float64)
    m = 0.5 * (a[0] + b[0])
    rms = lambda t: float(np.sqrt((t ** 2).mean()))
    rmse, rmse_merged, rms_res = rms(film - truth), rms(m - truth), rms(res)
    print(f"film_denoise quality {size} r {r} f {f} sigma {sigma}: rmse {rmse:.4e} merged {rmse_merged:.4e} ratio {rmse / rmse_merged:.3f} "
          f"residual rms / rmse {rms_res / rmse:.3f} mean shift {abs(film.mean() - m.mean()):.2e}")
    assert rmse <= 0.5 * rmse_merged
    assert abs(film.mean() - m.mean()) <= 1e-3
    assert 0.5 <= rms_res / rmse <= 2.0


# ---- the rest -----------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_say_why(scenes):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmDenoiseSpec, load_library
    W, H = SMALL
    sc = scenes[(W, H, 3)]
    a, b = denoise_films(H, W, 3, 1)
    call = lambda **kw: sc.film_denoise_host(a, SPE, b, SPE, **kw)
    with pytest.raises(WtgpuError, match=r"window_radius 11 out of range \(0 \.\. 10\)"):
        call(window=11)
    with pytest.raises(WtgpuError, match=r"patch_radius 4 out of range \(0 \.\. 3\)"):
        call(patch=4)
    for k in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(WtgpuError, match="a finite k > 0 expected"):
            call(k=k)
    for alpha in (-0.5, float("nan"), float("inf")):
        with pytest.raises(WtgpuError, match="a finite alpha >= 0 expected"):
            call(alpha=alpha)
    for eps in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(WtgpuError, match="a finite eps > 0 expected"):
            call(eps=eps)
    assert call(window=1, patch=0, alpha=0.0)["residual"] is None
    with pytest.raises(ValueError, match="films of the scene's size"):
        scenes[(W, H, 1)].film_denoise_host(a, SPE, b, SPE)
    with pytest.raises(ValueError, match="a mask of the scene's size"):
        call(mask=np.ones((H, W + 1), F32))
    # what the Python method cannot say: flags and null pointers go to the entry point itself
    lib = load_library()
    ptrs = [np.ascontiguousarray(t).ctypes.data for t in a + b]
    out = np.zeros((H, W, 3), F32)
    spec = FilmDenoiseSpec(1, 1, 4, 0, 0.45, 1.0, 1e-10, 0.0)
    assert lib.wtgpu_film_denoise_host(sc.handle, *ptrs[:3], SPE, *ptrs[3:], SPE, C.byref(spec), None, 1, out.ctypes.data, None) == 1
    assert b"no flags are defined" in lib.wtgpu_last_error()
    spec.flags = 0
    assert lib.wtgpu_film_denoise_host(sc.handle, *ptrs[:3], SPE, *ptrs[3:], SPE, C.byref(spec), None, 1, None, None) == 1
    assert b"null argument" in lib.wtgpu_last_error()
    assert lib.wtgpu_film_denoise_host(sc.handle, *ptrs[:3], SPE, *ptrs[3:], SPE, C.byref(spec), None, 1, out.ctypes.data, None) == 0 and out.any()


def test_render_denoise_on_numpy_films(scenes):
    from wave_tracer_amd.render import denoise
    W, H = SMALL
    sc = scenes[(W, H, 12)]
    a, b = films_with_bad_pixels(H, W, 12, 12)
    got = denoise(sc, a, b, SPE, window=3, patch=1)
    want = sc.film_denoise_host(a, SPE, b, SPE, window=3, patch=1, residual=True)
    assert same_bits(got["film"], want["film"]) and same_bits(got["residual"], want["residual"])
    film, res = want["film"][..., 0].astype(np.float64), want["residual"][..., 0].astype(np.float64)
    ok = np.isfinite(film).all(axis=-1) & np.isfinite(res).all(axis=-1)
    assert not ok.all() and got["residual_rel"] == pytest.approx(np.sqrt((res[ok] ** 2).sum() / (film[ok] ** 2).sum()), rel=1e-12) and 0 < got["residual_rel"] < 0.2
    bare = denoise(sc, a, b, SPE, window=3, patch=1, residual=False)
    assert bare["residual"] is None and bare["residual_rel"] is None and same_bits(bare["film"], want["film"])
    zero = (np.zeros((H, W, 12)), np.zeros((H, W)), np.zeros((H, W, 12)))
    assert denoise(sc, zero, zero, 1)["residual_rel"] == 0.0


def test_render_to_noise_keeps_the_halves(scenes):
    from test_film_compare import StubRenderer
    from wave_tracer_amd.render import denoise, render_to_noise
    sc = scenes[SMALL + (1,)]
    plain = render_to_noise(sc, 0.0, max_spp=14, chunk_spp=3, seed=9, renderer=StubRenderer())
    stub = StubRenderer()
    kept = render_to_noise(sc, 0.0, max_spp=14, chunk_spp=3, seed=9, renderer=stub, halves=True)
    assert len(plain) == 3 and len(kept) == 4 and kept[1:3] == plain[1:]
    assert all(same_bits(t, u) for t, u in zip(plain[0], kept[0]))                    # the default return value is unchanged
    half_a, half_b = kept[3]
    for t, x, y, parts in zip(kept[0], half_a, half_b, zip(*stub.films)):
        assert same_bits(x + y, t) and x is not t and y is not t                         # the halves sum to the merged film, and are copies
        assert same_bits(x, (parts[0] + parts[2]) + parts[4]) and same_bits(y, (parts[1] + parts[3]) + parts[5])
    got = denoise(sc, half_a, half_b, kept[1] // 2, window=2, patch=1)
    assert np.isfinite(got["film"]).all() and got["residual_rel"] > 0
