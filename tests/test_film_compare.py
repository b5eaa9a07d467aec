"""Film comparison (wt/film_compare.h: wtgpu_film_compare_host; render.noise_estimate, render.render_to_noise) on the CPU: the host twin against a
numpy restatement written here (it calls nothing of the library), on the synthetic films of tests/test_film_stats.py, whose developed values are
known exactly.  tests/test_gpu_film_compare.py runs the device kernels against the host twin on the same pairs.

What must agree exactly: the four counts, max_abs and argmax (the lowest pixel on a tie), the difference plane, and — the order of additions
being the fixed one of wt/film_stats.h — each of the five sums against a numpy restatement of that order, bit for bit.  Against math.fsum a sum is
held to n 2^-52 sum|addend|, the bound of tests/test_film_stats.py (f64 addition in ANY order: n - 1 roundings of at most 2^-53 of a partial
sum that never exceeds sum|addend|, with a factor 2 to spare); the addends themselves are restated operation by operation in f64, so they are
the library's."""
import ctypes as C
import math

import numpy as np
import pytest

from test_film_stats import LEVELS, PLANES, butterfly_sum, checker, elements, option_cases, restate_edges, same_bits, stats_films, stats_scene

F32 = np.float32
W, H = 37, 23
SPE_A, SPE_B = 7, 5
EDGES = restate_edges("dB", -50, 10, 4)        # (stats_films puts these values and their neighbours on the film)
NO_PIXEL = 2 ** 64 - 1
COUNTS = ("n", "n_nonfinite", "n_nonfinite_mismatch", "n_differ", "argmax")
SUMS = ("sum_abs", "sum_sq", "sum_a_sq", "sum_b_sq", "sum_rel")
FIELDS = COUNTS + ("max_abs",) + SUMS
QUIET_NAN = np.array([0x7fc00000], np.uint32).view(F32)[0]


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_compare")
    return {P: stats_scene(d, P) for P in PLANES}


def films_of(P, seed, height=H, width=W):
    _, _, channels, stokes = PLANES[P]
    return stats_films(height, width, channels, stokes, seed, EDGES)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def restate_compare(xa, xb, mask, eps):
    """xa, xb: [pixels, planes] f32 (test_film_stats.elements) -> the records Scene.film_compare_host returns, the sums in the fixed order
    ("<name>"), by math.fsum ("<name>_fsum") and the bound between the two ("<name>_bound"), and the difference plane."""
    inc = np.ones(len(xa), bool) if mask is None else (mask.reshape(-1) > 0)
    out = {k: [] for k in FIELDS + tuple(f"{s}_{t}" for s in SUMS for t in ("fsum", "bound"))}
    with np.errstate(all="ignore"):
        d32 = xa - xb
    out["diff"] = np.where(inc[:, None], np.where(np.isnan(d32), QUIET_NAN, d32), F32(0))
    for c in range(xa.shape[1]):
        a, b = xa[:, c], xb[:, c]
        fin = np.isfinite(a) & np.isfinite(b)
        nonfinite, take = inc & ~fin, inc & fin
        A, B = np.where(take, a.astype(np.float64), 0.0), np.where(take, b.astype(np.float64), 0.0)
        d = A - B
        out["n"].append(int(inc.sum()))
        out["n_nonfinite"].append(int(nonfinite.sum()))
        out["n_nonfinite_mismatch"].append(int((nonfinite & ~((np.isnan(a) & np.isnan(b)) | (a == b))).sum()))
        out["n_differ"].append(int((take & (a != b)).sum()))
        out["max_abs"].append(float(np.abs(d).max()))
        out["argmax"].append(int(np.argmax(np.abs(d))) if np.abs(d).max() > 0 else NO_PIXEL)      # (argmax: the first of equal maxima)
        for name, addend in zip(SUMS, (np.abs(d), d * d, A * A, B * B, d * d / (B * B + eps))):
            out[name].append(butterfly_sum(addend))
            out[name + "_fsum"].append(math.fsum(addend.tolist()))
            out[name + "_bound"].append(out["n"][-1] * 2.0 ** -52 * math.fsum(np.abs(addend).tolist()))
    return out


def check_against_restatement(got, want, label):
    for name in COUNTS:
        assert got[name].dtype == np.uint64 and got[name].tolist() == want[name], (label, name, got[name].tolist(), want[name])
    assert same_bits(got["max_abs"], np.array(want["max_abs"])), (label, "max_abs", got["max_abs"], want["max_abs"])
    for name in SUMS:
        assert same_bits(got[name], np.array(want[name], dtype=np.float64)), (label, name, "against the restated order", got[name], want[name])
        for c, (s, f, bound) in enumerate(zip(got[name], want[name + "_fsum"], want[name + "_bound"])):
            assert abs(s - f) <= bound, (label, name, c, s, f, bound)
    if "diff" in got:
        assert same_bits(got["diff"].reshape(want["diff"].shape), want["diff"]), (label, "diff")


def pairs(P):
    """(label, films A, films B) of the cases every plane count is held to: two draws; a film against itself; against a copy with one element
    of plane 0 moved by one f32 ulp (pixel 500: weight 1, no light, so the developed value moves by that ulp)."""
    a, b = films_of(P, 300 + P), films_of(P, 400 + P)
    one = tuple(t.copy() for t in a)
    v = one[0].reshape(H * W, -1)
    assert one[1].reshape(-1)[500] == 1.0 and np.isfinite(v[500, 0])
    v[500, 0] = float(np.nextafter(F32(v[500, 0]), F32(np.inf)))
    return [("two draws", a, b), ("itself", a, a), ("one ulp", a, one)]


# ---- the host twin against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(PLANES))
def test_host_twin_equals_the_restatement(scenes, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    mask = checker(H, W)
    for label, fa, fb in pairs(P):
        for s, abs_, lum, masked in option_cases(channels, stokes):
            if label == "one ulp" and s != 0:
                continue
            m = mask if masked else None
            eps = 1e-4 if s % 2 == 0 else 3e-9
            got = sc.film_compare_host(fa, SPE_A, fb, SPE_B if label == "two draws" else SPE_A, stokes_component=s, abs=abs_, luminance=lum, mask=m, eps=eps, diff=True,
                                       threads=3)
            xa = elements(channels, stokes, fa, SPE_A, s, abs_, lum)
            xb = elements(channels, stokes, fb, SPE_B if label == "two draws" else SPE_A, s, abs_, lum)
            want = restate_compare(xa, xb, m, eps)
            case = (P, label, s, abs_, lum, masked)
            assert got["diff"].dtype == F32 and got["diff"].shape == (H, W, channels + lum), case
            check_against_restatement(got, want, case)
            assert (got["n"] == (H * W if m is None else int((m > 0).sum()))).all()
            if label == "two draws":     # the films were built to meet every class: NaN against NaN, infinities of equal and of opposite sign against finite values
                assert got["n_nonfinite"].all() and got["n_differ"].all() and (got["max_abs"] > 0).all(), case
            if label == "itself":
                # (a film against itself has the NaN and the infinities at the same places: non-finite pairs, none of them a mismatch; the sums
                # of the DIFFERENCE are zero, the two sums of squares are each other's)
                assert got["n_nonfinite"].all() or masked, case
                for name in ("n_nonfinite_mismatch", "n_differ", "max_abs", "sum_abs", "sum_sq", "sum_rel"):
                    assert not got[name].any(), (case, name)
                assert (got["argmax"] == NO_PIXEL).all() and same_bits(got["sum_a_sq"], got["sum_b_sq"]) and not got["diff"][np.isfinite(got["diff"])].any(), case
            if label == "one ulp":
                moved = not masked or mask.reshape(-1)[500] > 0
                assert got["n_differ"][0] == int(moved) and got["argmax"][0] == (500 if moved else NO_PIXEL), case
                assert not got["n_differ"][1:channels].any() and (got["argmax"][1:channels] == NO_PIXEL).all(), case


def test_host_twin_equals_the_restatement_over_two_levels(built, tmp_path):
    """At LEVELS (test_film_stats.py) the loop over the levels runs twice and its second pass reads what the first wrote.  Two draws of an RGB
    film with its luminance under the checker mask, every field and the difference plane."""
    w, h = LEVELS
    sc = stats_scene(tmp_path, 3, w, h)
    mask = checker(h, w)
    fa, fb = films_of(3, 800, h, w), films_of(3, 801, h, w)
    got = sc.film_compare_host(fa, SPE_A, fb, SPE_B, luminance=True, mask=mask, diff=True, threads=3)
    want = restate_compare(elements(3, 1, fa, SPE_A, 0, False, True), elements(3, 1, fb, SPE_B, 0, False, True), mask, 1e-4)
    assert got["diff"].shape == (h, w, 4) and (got["n"] == int((mask > 0).sum())).all()
    check_against_restatement(got, want, LEVELS)
    assert got["n_nonfinite"].all() and got["n_differ"].all() and all(got[name].all() for name in SUMS)


def test_two_draws_meet_a_mismatch(scenes):
    """stats_films puts +inf and -inf at fixed pixels: the same draw with the planes negated meets -inf against +inf (a mismatch) and NaN against
    NaN (none)."""
    sc = scenes[3]
    a = films_of(3, 7)
    b = (-a[0], a[1], -a[2])
    got = sc.film_compare_host(a, SPE_A, b, SPE_A)
    check_against_restatement(got, restate_compare(elements(3, 1, a, SPE_A, 0, False, False), elements(3, 1, b, SPE_A, 0, False, False), None, 1e-4), "negated")
    assert (got["n_nonfinite"] == 3).all() and (got["n_nonfinite_mismatch"] == 2).all()
    both = sc.film_compare_host(a, SPE_A, b, SPE_A, abs=True)       # |x| against |-x|: nothing differs, the infinities are equal
    assert not both["n_differ"].any() and not both["n_nonfinite_mismatch"].any() and (both["argmax"] == NO_PIXEL).all()


def test_a_tie_for_the_maximum_goes_to_the_lowest_pixel(scenes):
    sc = scenes[1]
    a = (np.ones((H, W, 1)), np.ones((H, W)), np.zeros((H, W, 1)))
    for pixels in ([700, 300, 555], [850, 849], [0, 256]):       # in different chunks, in one chunk, first elements of two chunks
        b = tuple(t.copy() for t in a)
        b[0].reshape(-1)[pixels] = 1.5
        b[0].reshape(-1)[pixels[0]] = 0.5                          # the same |d| with the other sign
        for threads in (1, 5):
            got = sc.film_compare_host(a, 0, b, 0, threads=threads)
            assert got["max_abs"][0] == 0.5 and got["argmax"][0] == min(pixels) and got["n_differ"][0] == len(pixels) and got["sum_abs"][0] == 0.5 * len(pixels)
    m = np.ones((H, W), F32)
    m.reshape(-1)[300] = 0                                         # ... of the INCLUDED pixels
    b = tuple(t.copy() for t in a)
    b[0].reshape(-1)[[700, 300, 555]] = 1.5
    assert sc.film_compare_host(a, 0, b, 0, mask=m)["argmax"][0] == 555


EARLY, LATE = 3 * 256 + 17, 256 * 256 + 100      # at LEVELS: a pixel of chunk 3, and one of the last of the 257 chunks


def late_tie_films(early):
    """RGB films at LEVELS whose largest |d| = 2 of plane c is at pixel LATE + c and, with `early`, with the other sign at EARLY + c as well;
    every 97th pixel differs by 0.25, so that every chunk has a candidate of its own.  On the device the 257 chunks are those of 260 wavefronts,
    more records than the finish kernel's block has threads: the late pixel's is merged in its loop's second round (tests/test_gpu_film_compare.py)."""
    w, h = LEVELS
    a = (np.ones((h, w, 3)), np.ones((h, w)), np.zeros((h, w, 3)))
    b = tuple(t.copy() for t in a)
    v = b[0].reshape(h * w, 3)
    v[::97] = 1.25
    assert LATE // 256 == 256 and LATE + 2 < h * w and all(p % 97 for p in range(EARLY, EARLY + 3)) and all(p % 97 for p in range(LATE, LATE + 3))
    for c in range(3):
        v[LATE + c, c] = 3.0
        if early:
            v[EARLY + c, c] = -1.0
    return a, b


def test_a_late_maximum_and_a_tie_across_the_wavefronts_records(built, tmp_path):
    """The maximum in the last chunk and its equal in chunk 3: argmax is the smaller pixel; without the early one, the late pixel."""
    w, h = LEVELS
    sc = stats_scene(tmp_path, 3, w, h)
    for early in (True, False):
        a, b = late_tie_films(early)
        want = restate_compare(elements(3, 1, a, SPE_A, 0, False, False), elements(3, 1, b, SPE_A, 0, False, False), None, 1e-4)
        assert want["argmax"] == [(EARLY if early else LATE) + c for c in range(3)] and want["max_abs"] == [2.0] * 3      # the restatement alone
        for threads in (1, 5):
            check_against_restatement(sc.film_compare_host(a, SPE_A, b, SPE_A, threads=threads), want, ("late tie", early, threads))


def test_nothing_included(scenes):
    sc = scenes[3]
    mask = np.zeros((H, W), F32)
    mask[0, 0] = np.nan
    got = sc.film_compare_host(films_of(3, 1), SPE_A, films_of(3, 2), SPE_B, luminance=True, mask=mask, diff=True)
    for name in FIELDS:
        assert got[name].shape == (4,) and (got[name] == (NO_PIXEL if name == "argmax" else 0)).all(), name
    assert same_bits(got["diff"], np.zeros((H, W, 4), F32))
    assert np.isnan(got["rmse"]).all() and np.isnan(got["rel_l2"]).all()       # nothing to divide by


def test_the_result_does_not_depend_on_the_threads(scenes):
    for P in (3, 12):
        a, b = films_of(P, 9), films_of(P, 10)
        x, y = (scenes[P].film_compare_host(a, SPE_A, b, SPE_B, luminance=True, mask=checker(H, W), diff=True, threads=t) for t in (1, 5))
        assert all(same_bits(x[k], y[k]) for k in FIELDS + ("diff", "rmse", "mean_abs", "rel_l2", "rel_mse"))


def test_derived_values(scenes):
    sc = scenes[3]
    got = sc.film_compare_host(films_of(3, 1), SPE_A, films_of(3, 2), SPE_B, luminance=True)
    finite = (got["n"] - got["n_nonfinite"]).astype(np.float64)
    assert finite.all() and got["rmse"].shape == (4,)
    assert same_bits(got["rmse"], np.sqrt(got["sum_sq"] / finite)) and same_bits(got["mean_abs"], got["sum_abs"] / finite)
    assert same_bits(got["rel_l2"], np.sqrt(got["sum_sq"] / got["sum_b_sq"])) and same_bits(got["rel_mse"], got["sum_rel"] / finite)


def test_refusals_say_why(scenes):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmCompare, FilmCompareSpec, load_library
    mono, rgb = scenes[1], scenes[3]
    fm, fr = films_of(1, 1), films_of(3, 1)
    with pytest.raises(WtgpuError, match=r"film_compare: stokes_component 1 out of range \(the film has 1\)"):
        mono.film_compare_host(fm, 1, fm, 1, stokes_component=1)
    with pytest.raises(WtgpuError, match=r"film_compare: stokes_component 4 out of range \(the film has 4\)"):
        scenes[12].film_compare_host(films_of(12, 1), 1, films_of(12, 1), 1, stokes_component=4)
    with pytest.raises(WtgpuError, match=r"film_compare: LUMINANCE needs a 3-channel film \(this one has 1\)"):
        mono.film_compare_host(fm, 1, fm, 1, luminance=True)
    for eps in (0.0, -1e-4, float("nan"), float("inf")):
        with pytest.raises(WtgpuError, match="film_compare: a finite eps > 0 expected"):
            rgb.film_compare_host(fr, 1, fr, 1, eps=eps)
    with pytest.raises(ValueError, match="films of the scene's size"):
        rgb.film_compare_host(fr, 1, fm, 1)
    with pytest.raises(ValueError, match="a mask of the scene's size"):
        rgb.film_compare_host(fr, 1, fr, 1, mask=np.ones((H, W + 1), F32))
    # what the Python method cannot say: unknown flags and null pointers, at the entry point itself (WTGPU_ERR_INVALID = 1)
    lib = load_library()
    rec = (FilmCompare * 4)()
    p = [t.ctypes.data for t in fr]
    for spec, films_b, message in ((FilmCompareSpec(0, 4, 1e-4), p, b"film_compare: flags 1 (ABS) and 2 (LUMINANCE) expected"), (FilmCompareSpec(0, 0, 1e-4), [p[0], None, p[2]], b"null argument")):
        assert lib.wtgpu_film_compare_host(rgb.handle, *p, 1, *films_b, 1, C.byref(spec), None, 1, C.cast(rec, C.c_void_p), None) == 1
        assert message in lib.wtgpu_last_error()
    # spe = 0 is not refused: wtgpu_develop takes it as "no light term", and so does the comparison
    assert rgb.film_compare_host(fr, 0, fr, 0)["n"].tolist() == [H * W] * 3


# ---- render.noise_estimate, render.render_to_noise ------------------------------------------------------------------------------------------
def restate_noise(channels, films_a, films_b, spe, mask=None):
    """||a - b|| / ||a + b|| in f64 over the pairs of finite developed values of the luminance (RGB) or the one plane"""
    xa, xb = (elements(channels, 1, f, spe, 0, False, channels == 3)[:, -1].astype(np.float64) for f in (films_a, films_b))
    keep = np.isfinite(xa) & np.isfinite(xb) & (True if mask is None else mask.reshape(-1) > 0)
    xa, xb = xa[keep], xb[keep]
    return math.sqrt(math.fsum(((xa - xb) ** 2).tolist()) / math.fsum(((xa + xb) ** 2).tolist()))


def test_noise_estimate_is_the_formula(scenes):
    from wave_tracer_amd.render import noise_estimate
    for P, channels in ((1, 1), (3, 3)):
        sc = scenes[P]
        a, b = films_of(P, 21), films_of(P, 22)
        for mask in (None, checker(H, W)):
            got = noise_estimate(sc, a, b, SPE_A, mask=mask)
            c = sc.film_compare_host(a, SPE_A, b, SPE_A, luminance=channels == 3, mask=mask)
            k = -1
            assert got == math.sqrt(c["sum_sq"][k] / (2 * c["sum_a_sq"][k] + 2 * c["sum_b_sq"][k] - c["sum_sq"][k]))
            # the sums are good to 851 x 2^-52 each; so is their quotient, with room to spare
            assert got == pytest.approx(restate_noise(channels, a, b, SPE_A, mask), rel=1e-12)
        zero = (np.zeros((H, W, channels)), np.zeros((H, W)), np.zeros((H, W, channels)))
        assert noise_estimate(sc, zero, zero, 1) == 0.0
        assert noise_estimate(sc, a, a, SPE_A) == 0.0


class StubRenderer:
    """Deterministic films per sample range: n = end - begin samples of weight 1 whose value is 1 + pattern / (1 + begin) with a fixed +-1
    pattern — a constant and a term that shrinks with the range's index, so that the two halves draw together as the pairs go by."""

    def __init__(self):
        self.calls, self.films = [], []
        self.pattern = np.where(checker(H, W) > 0, 1.0, -1.0).reshape(H, W, 1)

    def __call__(self, begin, end, seed):
        n = end - begin
        films = (n * (1.0 + self.pattern / (1.0 + begin)), np.full((H, W), float(n)), np.full((H, W, 1), 1e-3 * n))
        self.calls.append((begin, end, seed))
        self.films.append(tuple(t.copy() for t in films))
        return films


def test_render_to_noise_with_a_stub_renderer(scenes):
    from wave_tracer_amd.render import render_to_noise
    sc = scenes[1]
    stub = StubRenderer()
    films, spp, history = render_to_noise(sc, 0.0, max_spp=14, chunk_spp=3, seed=9, renderer=stub)
    # target 0 is never met: every pair is rendered, the last one shortened to what max_spp leaves, the halves alternate
    assert spp == 14 and stub.calls == [(0, 3, 9), (3, 6, 9), (6, 9, 9), (9, 12, 9), (12, 13, 9), (13, 14, 9)]
    assert [s for s, _ in history] == [6, 12, 14]
    for t, parts in zip(films, zip(*stub.films)):                  # A = its ranges in turn, B likewise, then A += B: the sum of what the stub returned
        assert np.array_equal(t, ((parts[0] + parts[2]) + parts[4]) + ((parts[1] + parts[3]) + parts[5]))
        assert np.allclose(t, sum(parts), rtol=1e-15, atol=0)
    # an estimate per pair, of the halves as they stood then
    for k, (s, est) in enumerate(history):
        a = tuple(sum(p) for p in zip(*stub.films[0:2 * k + 2:2]))
        b = tuple(sum(p) for p in zip(*stub.films[1:2 * k + 2:2]))
        assert est == pytest.approx(restate_noise(1, a, b, s // 2), rel=1e-12), k
    assert history[0][1] > history[1][1] > history[2][1] > 0
    # the first pair whose estimate meets the target is the last one rendered
    for k in range(3):
        again = StubRenderer()
        _, spp_k, hist_k = render_to_noise(sc, history[k][1], max_spp=14, chunk_spp=3, seed=9, renderer=again)
        assert hist_k == history[:k + 1] and spp_k == history[k][0] and len(again.calls) == 2 * (k + 1)
    _, spp_1, _ = render_to_noise(sc, 1e9, max_spp=14, chunk_spp=100, seed=9, renderer=StubRenderer())
    assert spp_1 == 14                                             # one pair of 7 + 7
    for bad in (7, 0, 1):
        with pytest.raises(ValueError, match="an even max_spp"):
            render_to_noise(sc, 0.0, max_spp=bad, renderer=StubRenderer())


def test_more_samples_give_a_smaller_estimate(built):
    """The CPU checker as the renderer: halves of 16 samples per element against halves of 1.  Variance scaling predicts a quarter of the
    estimate; asserted is only that it is smaller.  Measured with these seeds on the CPU: 0.5017 against 0.1622, a ratio of 0.32."""
    from oracle_util import oracle_render
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import noise_estimate
    sc = Scene("cornell_box", res=16, mesh_detail=0, lut=(32, 32))
    few = noise_estimate(sc, oracle_render(sc, 0, 1, 5)[:3], oracle_render(sc, 1, 2, 5)[:3], 1)
    many = noise_estimate(sc, oracle_render(sc, 0, 16, 5)[:3], oracle_render(sc, 16, 32, 5)[:3], 16)
    print(f"noise estimate: 1 + 1 samples {few:.4f}, 16 + 16 samples {many:.4f}, ratio {many / few:.3f}")
    assert 0 < many < few
