"""The polarisation view of a Stokes film (wt/film_polar.h: wtgpu_film_polar_host; render.polarisation) on the CPU: the host twin against a numpy
f64 restatement written here (it calls nothing of the library), on synthetic polarimetric films whose developed values are known exactly.
tests/test_gpu_film_polar.py runs the device kernels against the host twin on the same films.

What must agree exactly: the four counts, max_dop and argmax (the lowest pixel on a tie), the DOLP / DOP / DOCP / ANALYSER maps (np.sqrt is
correctly rounded, the order of operations is the header's) and — the order of additions being the fixed one of wt/film_stats.h — each of the six
sums against a numpy restatement of that order, bit for bit.  Against math.fsum a sum is held to n 2^-52 sum|addend|, the bound of
tests/test_film_stats.py.  The two angles come from the library's own arc tangent and are held to BOUND = 1e-8 + 1.2e-7 against
f32(np.arctan2 / 2): the 1e-8 asked of the polynomial (its header states < 1.2e-11) plus one f32 ulp at pi/2.  The largest difference seen is
printed and kept in tests/golden/polar_measured.json (POLAR_RECORD=<file> records it); an excess over BOUND is a finding, not a tolerance.
The picture is restated from the twin's own AOLP map (held to BOUND above) and the restated DOLP map."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from oracle_util import oracle_render
from test_film_stats import LEVELS, PLANES, butterfly_sum, checker, same_bits, stats_scene
from test_tonemap import F32, _apply, clamp01, quantise, restate_develop

W, H = 37, 23
MANY = (256, 192)
SPE = 7
NO_PIXEL = 2 ** 64 - 1
QUIET_NAN = np.array([0x7fc00000], np.uint32).view(F32)[0]
MAPS = ("dolp", "dop", "docp", "aolp", "chi", "analyser")
EXACT_MAPS = ("dolp", "dop", "docp", "analyser")
COUNTS = ("n", "n_nonfinite", "n_dark", "n_over", "argmax")
SUMS = ("sum_i", "sum_q", "sum_u", "sum_v", "sum_lin", "sum_pol")
FIELDS = COUNTS + ("max_dop",) + SUMS
DERIVED = ("dop_total", "aolp_total", "mean_dolp", "mean_dop")
BOUND = 1e-8 + 1.2e-7
THETA = 0.3
_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polar_measured.json")
POLAR = {4: 1, 12: 3}      # P of test_film_stats.PLANES -> channels


def note_measured(label, measured):
    """Prints the largest angle difference seen, holds it to BOUND, and records it (POLAR_RECORD=<file>) or checks that the committed table has it."""
    measured = float(measured)
    print(f"polar_measured {label}: {measured:.3e} (bound {BOUND:.3e})")
    assert measured <= BOUND, f"{label}: {measured:.3e} rad is above {BOUND:.3e}: a finding about pol_atan2, not a tolerance"
    out = os.environ.get("POLAR_RECORD")
    if out:
        try:
            with open(out) as f:
                rec = json.load(f)
        except (OSError, ValueError):
            rec = {}
        rec[label] = max(measured, rec.get(label, 0.0))
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        return
    with open(_TABLE) as f:
        assert label in json.load(f), f"{label}: no committed measurement in tests/golden/polar_measured.json (record one with POLAR_RECORD=<file>)"


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_polar")
    return {P: stats_scene(d, P) for P in PLANES}


# ---- films ------------------------------------------------------------------------------------------------------------------------------------
def _ulp(x, towards):
    return float(np.nextafter(F32(x), F32(towards)))


NAN, INF = float("nan"), float("inf")
SPECIAL = ([tuple(NAN if k == s else 0.25 for k in range(4)) for s in range(4)] +                # a NaN in each component (I = 0.25 otherwise: would be lit)
           [tuple(sign * INF if k == s else 0.25 for k in range(4)) for s in range(4) for sign in (1, -1)] +
           [(0.0, 0.0, 0.0, 0.0), (0.0, 0.5, -0.25, 0.125),                                        # I = 0: dark, whatever the rest says
            (-1.0, 0.25, 0.125, 0.0),                                                              # I < 0: dark
            (1.0, 0.0, 0.0, 0.5), (1.0, 0.0, 0.0, -0.5), (1.0, -0.0, -0.0, 0.5),                   # Q = U = 0 with V != 0: aolp = 0, chi = +-pi/4
            (1.0, -0.5, 0.0, 0.0), (1.0, -0.5, -0.0, 0.0),                                          # U = +-0 with Q < 0: aolp = +pi/2 both times
            (1.0, 0.0, 0.5, 0.125), (1.0, 0.0, -0.5, 0.0), (1.0, -0.0, 0.5, 0.0),                  # Q = 0: aolp = +-pi/4
            (1.0, _ulp(1, 2), 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (1.0, _ulp(1, 0), 0.0, 0.0),        # pol one ulp above I (over), equal, one ulp below
            (0.5, 0.0, 0.0, -_ulp(0.5, 1)), (0.5, 0.0, _ulp(0.5, 0), 0.0),
            (1.0, 0.5, 0.5, 0.0), (1.0, 0.5, 0.5 * (2 ** 0.5 - 1), 0.0), (1.0, -0.5, -0.5, 0.0)])  # the octants' and the reduction's borders
SPECIAL = SPECIAL + SPECIAL[:2]      # (pixels 1 and 3 are excluded by `checker`: what they hold is met again)


def polar_films(height, width, channels, seed):
    """Seeded polarimetric films [H,W,channels*4], [H,W], [H,W,channels*4] whose developed values are known f32: weight 1 and no light put `value`
    itself on the film.  Most pixels: physical Stokes vectors (pol <= I but for the rounding to f32) of log-uniform intensity, random angle and
    ellipticity; every eighth pixel has weight 0 (developed value: light / spe alone — a vector of its own for half of them, an exact 0, dark,
    for the rest).  The odd pixels from 1 on hold SPECIAL in every channel."""
    rng = np.random.default_rng(seed)
    n = height * width

    def vectors():
        i = 10.0 ** rng.uniform(-3.0, 1.0, (n, channels))
        p = i * np.where(rng.random((n, channels)) < 0.1, 1.0, rng.uniform(0.0, 1.0, (n, channels)))      # a tenth fully polarised: pol ~ I
        psi, chi = rng.uniform(-np.pi / 2, np.pi / 2, (n, channels)), rng.uniform(-np.pi / 4, np.pi / 4, (n, channels))
        s = np.stack((i, p * np.cos(2 * psi) * np.cos(2 * chi), p * np.sin(2 * psi) * np.cos(2 * chi), p * np.sin(2 * chi)), axis=-1)
        return s.astype(F32).astype(np.float64).reshape(n, channels * 4)

    value, weight, light = vectors(), np.ones(n), np.zeros((n, channels * 4))
    weight[::8] = 0.0
    value[::8] = rng.normal(size=(n, channels * 4))[::8]                               # (ignored: the weight is 0)
    light[::8] = (vectors() * SPE * (rng.random((n, 1)) < 0.5))[::8]
    assert n >= 2 * len(SPECIAL) + 2
    for k, e in enumerate(SPECIAL):
        value[2 * k + 1] = np.tile(np.array(e, dtype=np.float64), channels)
        light[2 * k + 1] = np.where(np.signbit(value[2 * k + 1]) & (value[2 * k + 1] == 0), -0.0, 0.0)     # (-0 + +0 = +0: a -0 needs both)
    return value.reshape(height, width, -1), weight.reshape(height, width), light.reshape(height, width, -1)


def stokes_of(films, channels, spe=SPE):
    """[pixels, channels, 4] f32: the developed Stokes vectors"""
    return restate_develop(*films, spe).reshape(-1, channels, 4)


def assert_films_hold_the_cases(x):
    """What polar_films placed by hand is on the developed film (plane 0), and at least 70 % of the pixels are lit."""
    i, q, u, v = (x[:, 0, s] for s in range(4))
    fin = np.isfinite(x[:, 0]).all(axis=1)
    for s in range(4):
        assert np.isnan(x[:, 0, s]).any() and (x[:, 0, s] == np.inf).any() and (x[:, 0, s] == -np.inf).any(), s
    assert (fin & (i == 0)).any() and (fin & (i < 0)).any()
    lit = fin & (i > 0)
    assert (lit & (q == 0) & (u == 0) & (v != 0)).any()
    assert (lit & (q < 0) & (u == 0) & ~np.signbit(u)).any() and (lit & (q < 0) & (u == 0) & np.signbit(u)).any()
    assert (lit & (q == 0) & (u != 0)).any()
    with np.errstate(all="ignore"):
        pol = np.sqrt((x[:, 0, 1:].astype(np.float64) ** 2).sum(axis=1))
    for target in (1.0, 0.5):
        assert (lit & (i == target) & (pol == _ulp(target, 2))).any() and (lit & (i == target) & (pol == _ulp(target, 0))).any(), target
    assert lit.mean() >= 0.7, lit.mean()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def restate_polar(x, luminance, mask, c2, s2):
    """x: [pixels, channels, 4] f32 -> the records Scene.film_polar_host returns, the sums in the fixed order ("<name>"), by math.fsum ("<name>_fsum")
    and the bound between the two ("<name>_bound"), the six maps [pixels, planes] (the angles by np.arctan2), and per plane `lit` and `I32`."""
    S = x.astype(np.float64)
    with np.errstate(all="ignore"):
        if luminance:
            S = np.concatenate((S, ((.2126 * S[:, 0] + .7152 * S[:, 1]) + .0722 * S[:, 2])[:, None]), axis=1)
        inc = np.ones(len(S), bool) if mask is None else (mask.reshape(-1) > 0)
        out = {k: [] for k in FIELDS + tuple(f"{s}_{t}" for s in SUMS for t in ("fsum", "bound")) + MAPS + ("lit", "I32")}
        for c in range(S.shape[1]):
            I, Q, U, V = (S[:, c, s] for s in range(4))
            fin = np.isfinite(S[:, c]).all(axis=1)
            lit = fin & (I > 0)
            i, q, u, v = np.where(lit, I, 1.0), np.where(lit, Q, 0.0), np.where(lit, U, 0.0), np.where(lit, V, 0.0)
            l2 = q * q + u * u
            p2 = l2 + v * v
            lin, pol = np.sqrt(l2), np.sqrt(p2)
            dop = pol / i
            values = {"dolp": lin / i, "dop": dop, "docp": v / i, "aolp": 0.5 * np.arctan2(u + 0.0, q + 0.0), "chi": 0.5 * np.arctan2(v + 0.0, lin),
                      "analyser": 0.5 * ((I + Q * c2) + U * s2)}
            for name in MAPS:
                m = np.where(lit | (fin & (name == "analyser")), values[name].astype(F32), F32(0))
                out[name].append(np.where(inc, np.where(fin, m, QUIET_NAN), F32(0)))
            take = inc & lit
            out["lit"].append(lit)
            out["I32"].append(I.astype(F32))
            out["n"].append(int(inc.sum()))
            out["n_nonfinite"].append(int((inc & ~fin).sum()))
            out["n_dark"].append(int((inc & fin & ~lit).sum()))
            out["n_over"].append(int((take & (p2 > i * i)).sum()))
            cand = np.where(take, dop, -1.0)
            out["max_dop"].append(float(cand.max()) if take.any() else 0.0)
            out["argmax"].append(int(np.argmax(cand)) if take.any() else NO_PIXEL)             # (argmax: the first of equal maxima)
            for name, addend in zip(SUMS, (i, q, u, v, lin, pol)):
                addend = np.where(take, addend, 0.0)
                out[name].append(butterfly_sum(addend))
                out[name + "_fsum"].append(math.fsum(addend.tolist()))
                out[name + "_bound"].append(out["n"][-1] * 2.0 ** -52 * math.fsum(np.abs(addend).tolist()))
    for name in MAPS + ("lit", "I32"):
        out[name] = np.stack(out[name], axis=1)
    out["inc"] = inc
    return out


def angle_excess(got, want, lit):
    """Largest |got - want| over the lit pixels of an angle map; everywhere else the two agree bit for bit (0, or the quiet NaN)."""
    assert same_bits(np.where(lit, F32(0), got), np.where(lit, F32(0), want))
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64))[lit].max()) if lit.any() else 0.0


def check_against_restatement(got, want, label, shape):
    """Every field and every map of `got` (a film_polar_host dict with all six maps) against restate_polar's; returns the largest angle difference."""
    for name in COUNTS:
        assert got[name].dtype == np.uint64 and got[name].tolist() == want[name], (label, name, got[name].tolist(), want[name])
    assert same_bits(got["max_dop"], np.array(want["max_dop"])), (label, "max_dop", got["max_dop"], want["max_dop"])
    for name in SUMS:
        assert same_bits(got[name], np.array(want[name], dtype=np.float64)), (label, name, "against the restated order", got[name], want[name])
        for c, (s, f, bound) in enumerate(zip(got[name], want[name + "_fsum"], want[name + "_bound"])):
            assert abs(s - f) <= bound, (label, name, c, s, f, bound)
    worst = 0.0
    for name in got["maps"]:
        m = got["maps"][name]
        assert m.dtype == F32 and m.shape == shape, (label, name, m.shape)
        if name in EXACT_MAPS:
            assert same_bits(m.reshape(want[name].shape), want[name]), (label, name)
        else:
            inc_lit = want["lit"] & want["inc"][:, None]
            worst = max(worst, angle_excess(m.reshape(want[name].shape), want[name], inc_lit))
    return worst


def restate_picture(want, aolp, plane, tm, sat_gain, T=F32):
    """The false-colour picture [pixels, 3] in number type T from the restated DOLP map and I, and the AOLP map `aolp` of the library (every pixel
    is shown, so all three must come from a call WITHOUT a mask); NaN where the value is NaN."""
    lit, i32 = want["lit"][:, plane], want["I32"][:, plane]
    with np.errstate(all="ignore"):
        hue = np.where(lit, (aolp[:, plane].astype(np.float64) / np.pi + 0.5).astype(F32), F32(0))
        sg = want["dolp"][:, plane] * F32(sat_gain)
        sat = np.where(lit & ~np.isnan(sg), clamp01(sg), F32(0))
        val = clamp01(_apply(tm, i32.astype(T), T))
        hue, sat = hue.astype(T), sat.astype(T)
        h6 = hue * T(6)
        sextant = np.minimum(np.where(np.isnan(h6), 0, h6).astype(np.int64), 5)
        f = h6 - sextant.astype(T)
        p, q, t = val * (T(1) - sat), val * (T(1) - sat * f), val * (T(1) - sat * (T(1) - f))
        table = {"r": (val, q, p, p, t, val), "g": (t, val, val, q, p, p), "b": (p, p, t, val, val, q)}
        rgb = np.stack([np.choose(sextant, table[k]) for k in "rgb"], axis=1)
    rgb[np.isnan(val)] = QUIET_NAN if T is F32 else np.nan
    return rgb


def with_alpha(rgb, mask, fmt):
    if mask is None:
        return rgb
    a = mask.reshape(-1, 1)
    return np.concatenate((rgb, a if fmt == "f32" else quantise(a, fmt).astype(rgb.dtype)), axis=1)


def codes(rgb, fmt):
    return rgb if fmt == "f32" else quantise(rgb, fmt).astype({"u8": np.uint8, "u16": np.uint16}[fmt])


# ---- the host twin against the restatement ----------------------------------------------------------------------------------------------------
def _one_film(sc, P, width, height, seed, label):
    channels = POLAR[P]
    films = polar_films(height, width, channels, seed)
    x = stokes_of(films, channels)
    assert_films_hold_the_cases(x)
    c2, s2 = math.cos(2 * THETA), math.sin(2 * THETA)
    worst = 0.0
    for lum in ((False, True) if channels == 3 else (False,)):
        for mask in (None, checker(height, width)):
            want = restate_polar(x, lum, mask, c2, s2)
            # the restatement alone: every class is met, in every plane
            assert all(want["n_nonfinite"]) and all(want["n_dark"]) and all(want["n_over"]), (label, lum, want["n_nonfinite"], want["n_dark"], want["n_over"])
            assert all(m < NO_PIXEL for m in want["argmax"]) and all(0 < m for m in want["max_dop"])
            got = sc.film_polar_host(*films, SPE, luminance=lum, maps=MAPS, analyser=THETA, mask=mask, threads=3)
            worst = max(worst, check_against_restatement(got, want, (label, P, lum, mask is not None), (height, width, channels + lum)))
            assert (got["n"] == (height * width if mask is None else int((mask > 0).sum()))).all()
            with np.errstate(all="ignore"):
                assert same_bits(got["dop_total"], np.sqrt(got["sum_q"] ** 2 + got["sum_u"] ** 2 + got["sum_v"] ** 2) / got["sum_i"])
                assert same_bits(got["aolp_total"], 0.5 * np.arctan2(got["sum_u"], got["sum_q"]))
                assert same_bits(got["mean_dolp"], got["sum_lin"] / got["sum_i"]) and same_bits(got["mean_dop"], got["sum_pol"] / got["sum_i"])
            assert (0 < got["mean_dolp"]).all() and (got["mean_dolp"] <= got["mean_dop"]).all() and (got["dop_total"] <= got["mean_dop"] * (1 + 1e-12)).all()
            # thread counts: the same bytes
            for threads in (1, 5):
                again = sc.film_polar_host(*films, SPE, luminance=lum, maps=MAPS, analyser=THETA, mask=mask, threads=threads)
                assert all(same_bits(again[k], got[k]) for k in FIELDS + DERIVED) and all(same_bits(again["maps"][m], got["maps"][m]) for m in MAPS)
    return worst


@pytest.mark.parametrize("P", sorted(POLAR))
def test_host_twin_equals_the_restatement(scenes, P):
    note_measured(f"films/{W}x{H}/P{P}", _one_film(scenes[P], P, W, H, 100 + P, "small"))


@pytest.mark.parametrize("P", sorted(POLAR))
def test_host_twin_equals_the_restatement_on_many_chunks(built, tmp_path, P):
    w, h = MANY
    note_measured(f"films/{w}x{h}/P{P}", _one_film(stats_scene(tmp_path, P, w, h), P, w, h, 200 + P, "many chunks"))


def test_host_twin_equals_the_restatement_over_two_levels(built, tmp_path):
    """At LEVELS (test_film_stats.py) the loop over the levels runs twice and its second pass reads what the first wrote."""
    w, h = LEVELS
    note_measured(f"films/{w}x{h}/P12", _one_film(stats_scene(tmp_path, 12, w, h), 12, w, h, 312, "two levels"))


EARLY, LATE = 3 * 256 + 17, 256 * 256 + 100      # at LEVELS: a pixel of chunk 3, and one of the last of the 257 chunks


def late_tie_films(early):
    """Polarimetric RGB films at LEVELS whose largest degree of polarisation, 0.75, of channel c is at pixel LATE + c (1, 0, .75, 0) and, with
    `early`, at EARLY + c as well, from other numbers (2, 0, 0, 1.5); dop is 0.25 elsewhere and 0.5 at every 97th pixel, so that every chunk has a
    candidate of its own.  On the device the 257 chunks are those of 260 wavefronts, more records than the finish kernel's block has threads: the
    late pixel's is merged in its loop's second round (tests/test_gpu_film_polar.py)."""
    w, h = LEVELS
    value = np.tile(np.array([1.0, 0.25, 0.0, 0.0]), (h * w, 3)).reshape(h * w, 3, 4)
    value[::97, :, 1] = 0.5
    assert LATE // 256 == 256 and LATE + 2 < h * w and all(p % 97 for p in range(EARLY, EARLY + 3)) and all(p % 97 for p in range(LATE, LATE + 3))
    for c in range(3):
        value[LATE + c, c] = (1.0, 0.0, 0.75, 0.0)
        if early:
            value[EARLY + c, c] = (2.0, 0.0, 0.0, 1.5)
    return value.reshape(h, w, 12), np.ones((h, w)), np.zeros((h, w, 12))


def test_a_late_maximum_and_a_tie_across_the_wavefronts_records(built, tmp_path):
    """The maximum in the last chunk and its equal in chunk 3: argmax is the smaller pixel; without the early one, the late pixel."""
    w, h = LEVELS
    sc = stats_scene(tmp_path, 12, w, h)
    for early in (True, False):
        films = late_tie_films(early)
        want = restate_polar(stokes_of(films, 3), False, None, 1.0, 0.0)
        assert want["argmax"] == [(EARLY if early else LATE) + c for c in range(3)] and want["max_dop"] == [0.75] * 3      # the restatement alone
        for threads in (1, 5):
            check_against_restatement(sc.film_polar_host(*films, SPE, threads=threads), want, ("late tie", early, threads), None)


def sweep_films(height, width):
    """An RGB polarimetric film of directions: (Q, U, V) = m (cos b cos a, cos b sin a, sin b), I = 2 m, with a over (-pi, pi], b over [-pi/2, pi/2] and
    m log-uniform from 1e-30 to 1e30 — 3 x pixels directions; the first pixels hold the borders of pol_atan2's reductions exactly."""
    rng = np.random.default_rng(77)
    n = height * width
    a, b = rng.uniform(-np.pi, np.pi, (n, 3)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 3))
    m = 10.0 ** rng.uniform(-30.0, 30.0, (n, 3))
    s = np.stack((2 * m, m * np.cos(b) * np.cos(a), m * np.cos(b) * np.sin(a), m * np.sin(b)), axis=-1)
    t = 2 ** 0.5 - 1
    borders = [(q, u, v) for q in (1.0, -1.0, 0.0, t, -t) for u in (1.0, -1.0, 0.0, -0.0, t, -t) for v in (0.0, 1.0, -t)]
    for k, (q, u, v) in enumerate(borders):
        s[k, :, :] = (4.0, q, u, v)
        s[k, 1] *= 1e-30
        s[k, 2] *= 1e30
    value = s.astype(F32).astype(np.float64).reshape(height, width, 12)
    return value, np.ones((height, width)), np.zeros((height, width, 12))


def test_angles_over_a_sweep_of_directions(built, tmp_path):
    """At least 1e5 directions at magnitudes from 1e-30 to 1e30: AOLP and CHI against f32(np.arctan2 / 2), held to BOUND."""
    w, h = MANY
    sc = stats_scene(tmp_path, 12, w, h)
    films = sweep_films(h, w)
    x = stokes_of(films, 3)
    assert 3 * w * h >= 100000 and np.isfinite(x).all() and (x[..., 0] > 0).all()
    mag = np.abs(x[..., 1].astype(np.float64))
    assert mag[mag > 0].min() < 1e-29 and mag.max() > 1e29
    want = restate_polar(x, False, None, 1.0, 0.0)
    got = sc.film_polar_host(*films, SPE, maps=("aolp", "chi"))
    assert want["lit"].all() and sorted(got["maps"]) == ["aolp", "chi"]
    worst = {name: angle_excess(got["maps"][name].reshape(-1, 3), want[name], want["lit"]) for name in ("aolp", "chi")}
    for name, m in worst.items():
        note_measured(f"sweep/{name}", m)
    assert (np.abs(got["maps"]["aolp"]) <= F32(np.pi / 2)).all() and (np.abs(got["maps"]["chi"]) <= F32(np.pi / 4)).all()


def test_the_zeros_and_the_borders_of_the_angle(scenes):
    """A zero of either sign counts as +0; lin == 0 gives aolp = 0; the exact directions give the exact f32 of their angle."""
    films = polar_films(H, W, 1, 9)
    x = stokes_of(films, 1)[:, 0]
    got = scenes[4].film_polar_host(*films, SPE, maps=("aolp", "chi"))["maps"]
    aolp, chi = got["aolp"].reshape(-1), got["chi"].reshape(-1)
    lit = np.isfinite(x).all(axis=1) & (x[:, 0] > 0)
    for sel, angle in (((x[:, 1] < 0) & (x[:, 2] == 0), np.pi / 2), ((x[:, 1] == 0) & (x[:, 2] > 0), np.pi / 4), ((x[:, 1] == 0) & (x[:, 2] < 0), -np.pi / 4),
                       ((x[:, 1] == 0) & (x[:, 2] == 0), 0.0), ((x[:, 1] > 0) & (x[:, 1] == x[:, 2]), np.pi / 8)):
        assert (lit & sel).any() and (aolp[lit & sel] == F32(angle)).all(), (angle, aolp[lit & sel])
    flat = lit & (x[:, 1] == 0) & (x[:, 2] == 0) & (x[:, 3] != 0)
    assert flat.any() and (chi[flat] == np.where(x[flat, 3] > 0, F32(np.pi / 4), F32(-np.pi / 4))).all()


def test_every_single_map_bit_and_all_six(scenes):
    """Each map alone is the slice of all six; no map: no maps."""
    for P in sorted(POLAR):
        films = polar_films(H, W, POLAR[P], 40 + P)
        lum = POLAR[P] == 3
        mask = checker(H, W)
        all_six = scenes[P].film_polar_host(*films, SPE, luminance=lum, maps=MAPS, analyser=THETA, mask=mask)
        for name in MAPS:
            one = scenes[P].film_polar_host(*films, SPE, luminance=lum, maps=name, analyser=THETA, mask=mask)
            assert list(one["maps"]) == [name] and same_bits(one["maps"][name], all_six["maps"][name]), (P, name)
            assert all(same_bits(one[k], all_six[k]) for k in FIELDS)
        pair = scenes[P].film_polar_host(*films, SPE, luminance=lum, maps=("analyser", "dop"), analyser=THETA, mask=mask)["maps"]
        assert list(pair) == ["dop", "analyser"] and all(same_bits(pair[k], all_six["maps"][k]) for k in pair)
        none = scenes[P].film_polar_host(*films, SPE, luminance=lum, mask=mask)
        assert none["maps"] == {} and none["picture"] is None and all(same_bits(none[k], all_six[k]) for k in FIELDS)
        assert not all_six["maps"]["analyser"][mask <= 0].any() and not all_six["maps"]["analyser"][np.isnan(mask)].any()


def test_a_mask_that_excludes_everything(scenes):
    for P in sorted(POLAR):
        films = polar_films(H, W, POLAR[P], 50 + P)
        mask = np.zeros((H, W), F32)
        mask[0, 0] = np.nan
        got = scenes[P].film_polar_host(*films, SPE, luminance=POLAR[P] == 3, maps=MAPS, mask=mask)
        want = restate_polar(stokes_of(films, POLAR[P]), POLAR[P] == 3, mask, 1.0, 0.0)
        check_against_restatement(got, want, (P, "nothing"), (H, W, POLAR[P] + (POLAR[P] == 3)))
        assert not any(got[k].any() for k in ("n", "n_nonfinite", "n_dark", "n_over", "max_dop") + SUMS) and (got["argmax"] == NO_PIXEL).all()
        assert not any(m.view(np.uint32).any() for m in got["maps"].values()) and np.isnan(got["mean_dop"]).all()


def test_the_luminance_is_linear_and_not_clamped(scenes):
    """The luminance plane of a film whose three channels hold the same vector S holds (.2126 + .7152) + .0722 times S component by component, also
    where I < 0 (dark: the analyser map shows it), and its sums are the channels' combined."""
    films = polar_films(H, W, 3, 61)
    got = scenes[12].film_polar_host(*films, SPE, luminance=True, maps=("analyser",), c2s2=(0.0, 0.0))
    x = stokes_of(films, 3).astype(np.float64)
    lum_i = (.2126 * x[:, 0, 0] + .7152 * x[:, 1, 0]) + .0722 * x[:, 2, 0]
    fin = np.isfinite(x).all(axis=(1, 2))
    a = got["maps"]["analyser"].reshape(-1, 4)[:, 3]
    assert (lum_i[fin] < 0).any() and same_bits(a[fin], (0.5 * lum_i[fin]).astype(F32))


# ---- the picture ------------------------------------------------------------------------------------------------------------------------------
PICTURE_TMS = [{"op": "gamma", "gamma": 2.2}, {"op": "sRGB"}, {"op": "dB", "db_range": (-30.0, 10.0)}]


@pytest.mark.parametrize("P", sorted(POLAR))
def test_the_picture_against_the_restatement(scenes, P):
    """Linear operator: bit for bit in f32, u8 and u16, RGB and RGBA.  sRGB, gamma, dB: within one code (the existing tonemap tests' rule)."""
    sc, channels = scenes[P], POLAR[P]
    films = polar_films(H, W, channels, 70 + P)
    x = stokes_of(films, channels)
    lum = channels == 3
    want = restate_polar(x, lum, None, 1.0, 0.0)
    aolp = sc.film_polar_host(*films, SPE, luminance=lum, maps="aolp")["maps"]["aolp"].reshape(H * W, -1)
    for plane in range(channels + lum):
        for sat_gain in (1.0, 2.5, 0.0):
            for mask in (None, checker(H, W)):
                for fmt in ("f32", "u8", "u16"):
                    got = sc.film_polar_host(*films, SPE, luminance=lum, mask=mask, picture=True, picture_plane=plane, fmt=fmt, sat_gain=sat_gain, threads=3)["picture"]
                    ref = with_alpha(codes(restate_picture(want, aolp, plane, {"op": "linear"}, sat_gain), fmt), mask, fmt)
                    assert got.shape == (H, W, 3 if mask is None else 4) and got.dtype == ref.dtype, (P, plane, fmt, got.dtype, ref.dtype)
                    assert same_bits(got.reshape(ref.shape), ref), (P, plane, sat_gain, mask is not None, fmt)
        colour = sc.film_polar_host(*films, SPE, luminance=lum, picture=True, picture_plane=plane, sat_gain=2.5)["picture"].reshape(-1, 3)
        vivid = want["lit"][:, plane] & (want["dolp"][:, plane] > 0.2)
        assert vivid.any() and (colour[vivid].max(axis=1) > colour[vivid].min(axis=1)).all()            # polarised light has a colour
        grey = ~want["lit"][:, plane] & np.isfinite(want["I32"][:, plane])
        assert grey.any() and (colour[grey, 0] == colour[grey, 1]).all() and (colour[grey, 1] == colour[grey, 2]).all()
        for tm in PICTURE_TMS:
            ref64 = restate_picture(want, aolp, plane, tm, 1.5, np.float64)
            for fmt in ("u8", "u16"):
                got = sc.film_polar_host(*films, SPE, luminance=lum, picture=True, picture_plane=plane, tm=tm, fmt=fmt, sat_gain=1.5)["picture"].astype(np.int64)
                assert np.abs(got.reshape(-1, 3) - quantise(ref64, fmt)).max() <= 1, (P, plane, tm, fmt)
                assert not got.reshape(-1, 3)[np.isnan(ref64)].any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_say_why(scenes):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmPolar, FilmPolarSpec, load_library
    from test_film_stats import restate_edges, stats_films
    for P in (1, 3):
        _, _, channels, stokes = PLANES[P]
        with pytest.raises(WtgpuError, match=r"a polarimetric film expected \(this one has 1 Stokes component\)"):
            scenes[P].film_polar_host(*stats_films(H, W, channels, stokes, 1, restate_edges("dB", -50, 10, 4)), SPE)
    mono, rgb = scenes[4], scenes[12]
    fm, fr = polar_films(H, W, 1, 1), polar_films(H, W, 3, 1)
    with pytest.raises(WtgpuError, match=r"LUMINANCE needs a 3-channel film \(this one has 1\)"):
        mono.film_polar_host(*fm, SPE, luminance=True)
    for c2s2 in ((float("nan"), 0.0), (1.0, float("inf"))):
        with pytest.raises(WtgpuError, match="finite c2 and s2 expected"):
            rgb.film_polar_host(*fr, SPE, c2s2=c2s2)
    for gain in (float("nan"), float("inf"), -0.5):
        with pytest.raises(WtgpuError, match="a finite sat_gain >= 0 expected"):
            rgb.film_polar_host(*fr, SPE, sat_gain=gain)
    with pytest.raises(WtgpuError, match=r"picture_plane 3 out of range \(the call has 3\)"):
        rgb.film_polar_host(*fr, SPE, picture=True, picture_plane=3)
    with pytest.raises(WtgpuError, match=r"picture_plane 1 out of range \(the call has 1\)"):
        mono.film_polar_host(*fm, SPE, picture_plane=1)
    assert rgb.film_polar_host(*fr, SPE, luminance=True, picture=True, picture_plane=3)["picture"].shape == (H, W, 3)
    with pytest.raises(WtgpuError, match="'function' operator is not supported"):
        rgb.film_polar_host(*fr, SPE, picture=True, tm={"op": "function"})
    with pytest.raises(WtgpuError, match="'gamma' must be positive"):
        rgb.film_polar_host(*fr, SPE, picture=True, tm={"op": "gamma", "gamma": 0.0})
    with pytest.raises(WtgpuError, match="valid 'db' range"):
        rgb.film_polar_host(*fr, SPE, picture=True, tm={"op": "dB", "db_range": (3.0, 3.0)})
    with pytest.raises(ValueError, match="maps of"):
        rgb.film_polar_host(*fr, SPE, maps=("dolp", "aop"))
    with pytest.raises(ValueError, match="fmt"):
        rgb.film_polar_host(*fr, SPE, picture=True, fmt="u32")
    with pytest.raises(ValueError, match="films of the scene's size"):
        rgb.film_polar_host(*fm, SPE)
    # what the Python method cannot say: unknown bits, formats and operators go to the entry point itself
    lib = load_library()
    v, w, l = (np.ascontiguousarray(t) for t in fr)

    def raw(**kw):
        spec, rec = FilmPolarSpec(), (FilmPolar * 4)()
        spec.c2 = 1.0
        for k, val in kw.items():
            if k == "op":
                spec.tonemap.op = val
            else:
                setattr(spec, k, val)
        rc = lib.wtgpu_film_polar_host(rgb.handle, v.ctypes.data, w.ctypes.data, l.ctypes.data, SPE, C.byref(spec), None, 1, C.cast(rec, C.c_void_p), None, None)
        return rc, lib.wtgpu_last_error().decode()
    assert raw()[0] == 0
    for kw, message in (({"flags": 1}, "flag 2 (LUMINANCE) expected"), ({"flags": 6}, "flag 2 (LUMINANCE) expected"), ({"maps": 64}, "map bits 1 (DOLP), 2 (DOP), 4 (DOCP), 8 (AOLP), 16 (CHI) and 32 (ANALYSER) expected"),
                        ({"format": 3}, "format 0 (f32), 1 (u8) or 2 (u16) expected"), ({"op": 5}, "operator 0 (linear), 1 (gamma), 2 (sRGB) or 3 (dB) expected"),
                        ({"op": -1}, "operator 0 (linear)")):
        rc, said = raw(**kw)
        assert rc == 1 and message in said, (kw, rc, said)
    maps = np.zeros(4, F32)
    spec, rec = FilmPolarSpec(), (FilmPolar * 4)()
    assert lib.wtgpu_film_polar_host(rgb.handle, v.ctypes.data, w.ctypes.data, l.ctypes.data, SPE, C.byref(spec), None, 1, C.cast(rec, C.c_void_p), maps.ctypes.data, None) == 1
    assert b"maps without a map bit" in lib.wtgpu_last_error()
    assert lib.wtgpu_film_polar_host(rgb.handle, v.ctypes.data, None, l.ctypes.data, SPE, C.byref(spec), None, 1, C.cast(rec, C.c_void_p), None, None) == 1
    assert b"null argument" in lib.wtgpu_last_error()


def test_polarisation_dispatches_on_the_films(scenes):
    from wave_tracer_amd.render import polarisation
    films = polar_films(H, W, 3, 3)
    a = polarisation(scenes[12], films, SPE, luminance=True, maps=("dop",), analyser=THETA)
    b = scenes[12].film_polar_host(*films, SPE, luminance=True, maps=("dop",), analyser=THETA)
    assert all(same_bits(a[k], b[k]) for k in FIELDS + DERIVED) and same_bits(a["maps"]["dop"], b["maps"]["dop"])


# ---- rendered films (the CPU checker's) -----------------------------------------------------------------------------------------------------
def test_rendered_films_of_the_cpu_checker(built):
    """cornell_box polarimetric (the arguments of tests/test_polarimetric.py): dielectric and conductor reflections polarise, and nothing is NaN;
    furnace_path polarimetric: Lambertian surfaces depolarise completely."""
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import polarisation
    sc = Scene("cornell_box", polarimetric=1, res=24, mesh_detail=0, crop_of=1440, lut=(64, 64))
    got = polarisation(sc, oracle_render(sc, 0, 8, 3)[:3], 8, luminance=True, maps=("dolp", "aolp"))
    assert (got["mean_dolp"] > 0).all() and not got["n_nonfinite"].any() and (got["n"] == sc.width * sc.height).all() and (got["max_dop"] > 0).all()
    assert (got["maps"]["dolp"] >= 0).all() and got["maps"]["dolp"].shape == (sc.height, sc.width, 4)
    sc = Scene("furnace_path", polarimetric=1, res=16)
    got = polarisation(sc, oracle_render(sc, 0, 4, 3)[:3], 4, luminance=sc.spectral_channels == 3, maps=("dop", "dolp", "docp"))
    assert (got["sum_i"] > 0).all() and not any(got[k].any() for k in ("sum_q", "sum_u", "sum_v", "sum_lin", "sum_pol", "n_nonfinite", "n_over", "max_dop"))
    assert not any(m.any() for m in got["maps"].values())
