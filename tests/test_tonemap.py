"""Film development and tonemapping (wt/tonemap.h; tonemap_t, src/sensor/response/tonemap.cpp) on the CPU: the scene reader's <tonemap>, and
wtgpu_tonemap_host against a numpy restatement of the reference's formulas written here (it calls nothing of the library).
tests/test_gpu_develop.py runs the device kernels against the same restatement and against the host twin.

The restatement works in a number type T.  With T = float32 it performs the reference's f32 operations one by one (numpy rounds after every
operation, nothing is fused): where the operator calls no libm function the library must agree with it BIT FOR BIT.  With T = float64 it is the
yardstick of gamma / sRGB / dB, whose powf / logf differ between libms: outputs lie in [0, 1] and f32 libm is good to a few ulp (6e-8 each), so
the differences should be of order 1e-6; the tolerance is 10 x the largest difference MEASURED over the films below (tests/golden/
tonemap_measured.json: "host/..." measured on the CPU, "device/..." on the MI355X), and a measurement above 1e-5 fails whatever the table says."""
import json
import math
import os

import numpy as np
import pytest

from test_sensor_mask import _write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLE = os.path.join(ROOT, "tests", "golden", "tonemap_measured.json")
ALARM = 1e-5     # the derivation says ~1e-6: anything above this is a finding, not a tolerance
FLOOR = 6e-8     # one ulp of an output near 1: a measured 0 does not demand bit equality of two libms
F32 = np.float32


def check_measured(label, measured):
    """measured <= 10 x the committed measurement of `label` and <= ALARM (the convention of tests/parity.py).  TONEMAP_RECORD=<file> records
    instead (a JSON file at that path, the maximum per label: merge it into the committed table); ALARM still applies."""
    measured = float(measured)
    print(f"tonemap_measured {label}: {measured:.3e}")
    assert measured <= ALARM, f"{label}: measured {measured:.3e} is above {ALARM:.0e}: f32 libm differences should be of order 1e-6"
    out = os.environ.get("TONEMAP_RECORD")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
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
        table = json.load(f)
    assert label in table, f"{label}: no committed measurement in tests/golden/tonemap_measured.json (record one with TONEMAP_RECORD=<file>); measured {measured:.3e}"
    tol = 10.0 * max(float(table[label]), FLOOR)
    assert measured <= tol, f"{label}: measured {measured:.3e}, tolerance {tol:.1e} = 10 x the committed measurement {float(table[label]):.3e}"


# ---- scene files ----------------------------------------------------------------------------------------------------------------------------
RGB = '<response type="RGB">{}</response>'
MONO = '<response type="monochromatic"><spectrum type="discrete" wavelength="550nm"/>{}</response>'


def film_xml(response=RGB, tonemap="", width=32, height=24, polarimetric=False):
    """A lit diffuse rectangle under a camera; what matters here is the film: its size, its response and the response's <tonemap>."""
    pol = ' polarimetric="true"' if polarimetric else ""
    source = ('<spectrum name="irradiance" type="discrete" wavelength="550nm" value="1"/>' if response == MONO else
              '<spectrum name="irradiance" blackbody="5500K"><float name="scale" value="5e-5"/></spectrum>')
    return f'''<scene version="0.1.0">
  <default name="db_min" value="-40"/><default name="db_max" value="-5"/>
  <integrator type="plt_path"><string name="direction" value="backward"/><integer name="max_depth" value="4"/></integrator>
  <sensor type="perspective"{pol}><quantity name="fov" value="60°"/>
    <transform name="to_world"><lookat origin="0m, 0m, 4m" target="0m, 0m, 0m" up="0, 1, 0"/></transform>
    <film type="array"><integer name="width" value="{width}"/><integer name="height" value="{height}"/>{response.format(tonemap)}</film></sensor>
  <emitter type="directional"><transform name="to_world"><lookat target="0m,0m,0m" origin="1m,2m,5m" up="0,1,0"/></transform>
    {source}</emitter>
  <bsdf type="diffuse" id="grey"><spectrum rgb="0.5, 0.5, 0.5" name="reflectance"/></bsdf>
  <shape type="rectangle" id="A"><point name="p" x="-20m" y="-20m" z="0m"/><point name="x" x="40m" y="0m" z="0m"/>
    <point name="y" x="0m" y="40m" z="0m"/><ref id="grey"/></shape>
</scene>'''


def _load(tmp_path, name, **kw):
    from wave_tracer_amd import Scene
    return Scene.from_xml(_write(tmp_path, name, film_xml(**kw)))


def test_spec_from_scene_files(built, tmp_path):
    """tonemap_t::load (tonemap.cpp:127-176): type, range, colourmap name, gamma, mode; what is not given keeps the loader's defaults (mode select,
    gamma 2.2, map Magma)."""
    db = _load(tmp_path, "db.xml", response=MONO, tonemap='<tonemap type="dB"><range value="$db_min .. $db_max"/><string name="colourmap" value="Turbo"/></tonemap>')
    assert db.tonemap_spec == {"present": True, "op": "dB", "mode": "select", "gamma": pytest.approx(2.2), "db_range": (-40.0, -5.0), "colourmap": "Turbo", "function": ""}
    g = _load(tmp_path, "g.xml", tonemap='<tonemap type="gamma"><float name="gamma" value="1.8"/></tonemap>').tonemap_spec
    assert (g["present"], g["op"], g["mode"], g["colourmap"]) == (True, "gamma", "select", "Magma") and g["gamma"] == pytest.approx(1.8)
    for mode in ("normal", "colourmap", "select"):
        m = _load(tmp_path, "m.xml", tonemap=f'<tonemap type="sRGB"><string name="mode" value="{mode}"/></tonemap>').tonemap_spec
        assert (m["op"], m["mode"]) == ("sRGB", mode)
    lin = _load(tmp_path, "l.xml", tonemap='<tonemap type="linear"/>').tonemap_spec
    assert lin["present"] and (lin["op"], lin["mode"]) == ("linear", "select")
    f = _load(tmp_path, "f.xml", tonemap='<tonemap type="function"><function value="sqrt(value)"/></tonemap>').tonemap_spec
    assert (f["op"], f["function"]) == ("function", "sqrt(value)")


@pytest.mark.parametrize("node,message", [
    ('<tonemap type="reinhard"/>', "(tonemap operator loader) Unrecognized 'type'"),
    ('<tonemap type="function"/>', "(tonemap operator loader) expected 'function' to be provided"),
    ('<tonemap type="dB"/>', "(tonemap operator loader) expected valid 'db' range to be provided"),
    ('<tonemap type="dB"><range value="-5 .. -40"/></tonemap>', "(tonemap operator loader) expected valid 'db' range to be provided"),
    ('<tonemap type="gamma"><float name="gamma" value="0"/></tonemap>', "(tonemap operator loader) 'gamma' must be positive"),
])
def test_the_loaders_error_messages(built, tmp_path, node, message):
    from wave_tracer_amd import WtgpuError
    with pytest.raises(WtgpuError) as e:
        _load(tmp_path, "bad.xml", tonemap=node)
    assert message in str(e.value)


def test_an_unqueried_child_is_warned_about(built, tmp_path, capfd):
    sc = _load(tmp_path, "w.xml", tonemap='<tonemap type="sRGB"><integer name="bits" value="8"/></tonemap>')
    assert sc.tonemap_spec["op"] == "sRGB"
    assert '(tonemap operator loader) Unqueried node type integer ("bits")' in capfd.readouterr().err


def test_defaults_without_a_node(built, tmp_path):
    """RGB response: sRGB / normal (RGB.cpp:91-93); monochromatic: linear / select (monochromatic.cpp:65-66); the map's name is Magma.  Bundled
    scenes report the default of their response."""
    from wave_tracer_amd import Scene
    rgb, mono = _load(tmp_path, "rgb.xml").tonemap_spec, _load(tmp_path, "mono.xml", response=MONO).tonemap_spec
    assert (rgb["present"], rgb["op"], rgb["mode"], rgb["colourmap"]) == (False, "sRGB", "normal", "Magma") and rgb["gamma"] == pytest.approx(2.2)
    assert (mono["present"], mono["op"], mono["mode"], mono["colourmap"]) == (False, "linear", "select", "Magma")
    for name, kw, want in (("furnace", {}, rgb), ("double_slits", {"lut": (32, 32)}, mono)):
        assert Scene(name, res=16, **kw).tonemap_spec == want


def test_a_tonemap_node_does_not_change_the_baked_scene(built, tmp_path):
    node = '<tonemap type="dB"><range value="$db_min .. $db_max"/><string name="colourmap" value="Turbo"/></tonemap>'
    for resp in (RGB, MONO):
        a, b = _load(tmp_path, "a.xml", response=resp, tonemap=node), _load(tmp_path, "b.xml", response=resp)
        assert a.first_difference(b) == "" and a.tonemap_spec["present"] and not b.tonemap_spec["present"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def clamp01(x):
    """glm::clamp = min(max(x, 0), 1) with max(x, y) = x < y ? y : x and min(x, y) = y < x ? y : x (math/common.hpp:508-511): NaN stays NaN."""
    y = np.where(x < 0, x.dtype.type(0), x)
    return np.where(1 < y, x.dtype.type(1), y)


def restate_develop(value, weight, light, spe):
    """render.cpp:245-291: value / weight (0 where the weight is 0) + light / spe in f64, then f32.  Films [H,W,P], [H,W], [H,W,P]."""
    sl = 1.0 / float(spe) if spe > 0 else 0.0
    with np.errstate(all="ignore"):
        v = np.where(weight[..., None] != 0, value / np.where(weight == 0, 1.0, weight)[..., None], 0.0)
        return (v + light * sl).astype(F32)


def _apply(tm, x, T):
    """tonemap.cpp:51-66 in number type T; the constants are the reference's f32 constants."""
    c = lambda k: T(F32(k))
    op = tm["op"]
    with np.errstate(all="ignore"):
        if op == "linear":
            return x
        if op == "gamma":
            return np.power(clamp01(x), T(F32(1) / F32(tm["gamma"])))
        if op == "sRGB":
            x = clamp01(x)
            return np.where(x <= c(.0031308), np.maximum(T(0), c(12.92) * x), c(1.055) * np.power(x, c(1. / 2.4)) - c(.055))
        assert op == "dB"
        lo, hi = F32(tm["db_range"][0]), F32(tm["db_range"][1])
        db = c(10. / math.log(10.)) * np.log(x)
        return np.where(x == 0, T(0), clamp01((db - T(lo)) / T(hi - lo)))


def _table_colour(table, v, T):
    n = len(table)
    tab = table.astype(T)
    c = clamp01(v)
    nan = np.isnan(c)
    pos = np.where(nan, T(0), c) * T(n - 1)
    i = np.minimum(pos.astype(np.int64), n - 2)
    f = (pos - i.astype(T))[..., None]
    out = tab[i] * (T(1) - f) + tab[i + 1] * f
    out[nan] = np.nan
    return out


def restate(channels, stokes, value, weight, light, spe, tm, s=0, T=np.float64):
    """tonemap_t::operator() (tonemap.cpp:72-106) on the developed planes of Stokes component s -> [H,W,3] in T.  tm: op, mode, gamma,
    db_range, table."""
    H, W = weight.shape
    d = restate_develop(value, weight, light, spe).reshape(H, W, channels, stokes)[..., s].astype(T)
    use_map = tm["mode"] == "colourmap" or (tm["mode"] == "select" and channels == 1)
    with np.errstate(all="ignore"):
        if use_map:
            if channels == 1:
                x = d[..., 0]
            else:   # RGB.hpp:155-157: max(0, dot), the three products added left to right; max(0, NaN) = 0
                lum = (T(F32(.2126)) * d[..., 0] + T(F32(.7152)) * d[..., 1]) + T(F32(.0722)) * d[..., 2]
                x = np.where(0 < lum, lum, T(0))
            return _table_colour(np.asarray(tm["table"], F32), _apply(tm, x, T), T)
        out = _apply(tm, d, T)
        return np.repeat(out, 3, axis=-1) if channels == 1 else out


def quantise(x, fmt):
    """(uint)(clamp01(x) max + 0.5); NaN is code 0."""
    mx = {"u8": 255, "u16": 65535}[fmt]
    c = clamp01(np.asarray(x))
    with np.errstate(all="ignore"):
        return np.where(np.isnan(c), 0, np.floor(np.where(np.isnan(c), 0, c) * c.dtype.type(mx) + c.dtype.type(.5))).astype(np.int64)


# ---- films ------------------------------------------------------------------------------------------------------------------------------------
DB_RANGE = (-60.0, 0.0)
EDGES = [0.0, -1.0, 1.0, float(np.nextafter(F32(1), F32(2))), float(F32(1e-45)), float("inf"), 1e-6, 1.0, float(F32(.0031308)), .5, .375, float("-inf")]


def make_films(H, W, channels, stokes, seed, kind="random"):
    """Seeded films [H,W,P], [H,W], [H,W,P] with developed values of both signs mostly in [-0.3, 1.3], weight 0 in every eighth pixel, and — for
    kind "edges" — the first pixels holding EDGES exactly in every plane (weight 1, no light): 0, -1, 1, just above 1, the smallest subnormal,
    inf, the two ends of DB_RANGE (1e-6 and 1), the sRGB knee, a position on entry 2 and halfway between entries 1 and 2 of a 5-entry table."""
    rng = np.random.default_rng(seed)
    P = channels * stokes
    weight = rng.uniform(0.5, 40.0, (H, W))
    weight.reshape(-1)[::8] = 0.0
    value = rng.uniform(-0.3, 1.3, (H, W, P)) * weight[..., None] + np.where(weight == 0, 1.0, 0.0)[..., None] * rng.normal(size=(H, W, P))
    light = rng.normal(scale=0.2, size=(H, W, P)) * (rng.random((H, W, P)) < 0.3)
    if kind == "no_light":
        light[:] = 0.0
    elif kind == "light_only":
        value[:] = 0.0
        weight[:] = 0.0
    elif kind == "edges":
        assert H * W >= 2 * len(EDGES) + 2
        for k, e in enumerate(EDGES):
            p = 2 * k + 1          # odd pixels: not the zero-weight ones
            value.reshape(-1, P)[p] = e
            weight.reshape(-1)[p] = 1.0
            light.reshape(-1, P)[p] = 0.0
    return value, weight, light


def grey_table(n=256):
    return (np.arange(n, dtype=np.float64) / (n - 1)).astype(F32)[:, None].repeat(3, axis=1)


def random_table(n, seed=5):
    return np.random.default_rng(seed).random((n, 3)).astype(F32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def nan_equal_maxdiff(got, want):
    """Largest |got - want| over the pixels where neither is NaN or infinite; NaNs and infinities must coincide."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN outputs differ"
    special = ~np.isfinite(want)
    assert np.array_equal(got[special & ~np.isnan(want)], want[special & ~np.isnan(want)]), "infinite outputs differ"
    return float(np.abs(got[~special] - want[~special]).max())


def scenes_by_planes():
    """Scenes chosen for their plane counts: (scene, channels, stokes) with P = 1, 3, 12, 4."""
    from wave_tracer_amd import Scene
    return [(Scene("double_slits", res=96, lut=(32, 32)), 1, 1), (Scene("cornell_box", res=32, mesh_detail=0, lut=(32, 32)), 3, 1),
            (Scene("cornell_box", res=32, mesh_detail=0, lut=(32, 32), polarimetric=1), 3, 4), (Scene("double_slits", res=96, lut=(32, 32), polarimetric=1), 1, 4)]


@pytest.fixture(scope="module")
def planes(built):
    return scenes_by_planes()


FILM_CASES = [("edges", 0), ("random", 7), ("no_light", 7), ("light_only", 7)]     # (kind, spe)
MODES = ["select", "normal", "colourmap"]


def test_libm_free_operators_are_bit_for_bit(planes):
    """linear in every mode, grey and random tables (5 and 256 entries), every Stokes component, every format, with and without the mask: the
    library equals the f32 restatement bit for bit; the alpha is the mask's bits (f32) or its code (u8 / u16)."""
    for sc, channels, stokes in planes:
        H, W = sc.height, sc.width
        assert (sc.spectral_channels, sc.stokes) == (channels, stokes)
        mask = np.random.default_rng(3).uniform(-0.2, 1.2, (H, W)).astype(F32)
        mask.reshape(-1)[:3] = [np.nan, 0.0, 1.0]
        for kind, spe in FILM_CASES:
            v, w, l = make_films(H, W, channels, stokes, 11, kind)
            for mode in MODES:
                for table in (grey_table(), random_table(5), random_table(256)):
                    tm = {"op": "linear", "mode": mode, "table": table}
                    for s in range(stokes):
                        want = restate(channels, stokes, v, w, l, spe, tm, s, T=F32)
                        got = sc.tonemap_host(v, w, l, spe, tm, s, threads=3)
                        assert got.dtype == F32 and same_bits(got, want), (sc.name, kind, mode, len(table), s)
                        if kind != "edges" or len(table) != 5:
                            continue
                        for fmt in ("u8", "u16"):
                            q = sc.tonemap_host(v, w, l, spe, tm, s, fmt=fmt)
                            assert np.array_equal(q.astype(np.int64), quantise(want, fmt)), (sc.name, mode, s, fmt)
                        for fmt in ("f32", "u8", "u16"):
                            q = sc.tonemap_host(v, w, l, spe, tm, s, mask=mask, fmt=fmt, threads=2)
                            assert q.shape == (H, W, 4)
                            if fmt == "f32":
                                assert same_bits(q[..., :3], want) and same_bits(q[..., 3], mask)
                            else:
                                assert np.array_equal(q[..., :3].astype(np.int64), quantise(want, fmt)) and np.array_equal(q[..., 3].astype(np.int64), quantise(mask, fmt))


def test_edge_values_come_out_as_the_reference_defines_them(planes):
    """The known pixels of the "edges" film, on the monochromatic film through a 5-entry table and per channel: clamp01 keeps NaN and maps
    negatives to 0; linear passes everything through; dB of 0 is 0, of a negative value NaN, of inf 1; table positions on and between entries."""
    sc, channels, stokes = planes[0]
    v, w, l = make_films(sc.height, sc.width, channels, stokes, 11, "edges")
    at = lambda img, e: img.reshape(-1, 3)[2 * EDGES.index(e) + 1]
    lin = sc.tonemap_host(v, w, l, 0, {"op": "linear", "mode": "normal"})
    for e in EDGES:
        assert same_bits(at(lin, e), np.full(3, e, F32))
    table = random_table(5)
    cm = sc.tonemap_host(v, w, l, 0, {"op": "linear", "mode": "colourmap", "table": table})
    assert same_bits(at(cm, .5), table[2]) and same_bits(at(cm, .375), table[1] * F32(.5) + table[2] * F32(.5))
    assert same_bits(at(cm, -1.0), table[0]) and same_bits(at(cm, float("inf")), table[4]) and same_bits(at(cm, 1.0), table[4])
    db = sc.tonemap_host(v, w, l, 0, {"op": "dB", "mode": "normal", "db_range": DB_RANGE})
    assert at(db, 0.0)[0] == 0 and np.isnan(at(db, -1.0)[0]) and at(db, float("inf"))[0] == 1 and at(db, 1.0)[0] == 1 and abs(at(db, 1e-6)[0]) < 1e-6
    assert np.isnan(at(db, float("-inf"))[0]) and at(db, float(F32(1e-45)))[0] == 0
    for fmt in ("u8", "u16"):
        assert at(sc.tonemap_host(v, w, l, 0, {"op": "dB", "mode": "normal", "db_range": DB_RANGE}, fmt=fmt), -1.0)[0] == 0      # NaN -> code 0
    srgb = sc.tonemap_host(v, w, l, 0, {"op": "sRGB", "mode": "normal"})
    knee = F32(.0031308)
    assert at(srgb, float(knee))[0] == F32(12.92) * knee and at(srgb, -1.0)[0] == 0 and at(srgb, float(np.nextafter(F32(1), F32(2))))[0] == at(srgb, 1.0)[0]
    g = sc.tonemap_host(v, w, l, 0, {"op": "gamma", "mode": "normal", "gamma": 2.2})
    assert at(g, 0.0)[0] == 0 and at(g, 1.0)[0] == 1 and at(g, float("inf"))[0] == 1 and at(g, -1.0)[0] == 0


LIBM_OPS = [{"op": "gamma", "gamma": 2.2}, {"op": "gamma", "gamma": 0.7}, {"op": "sRGB"}, {"op": "dB", "db_range": DB_RANGE}, {"op": "dB", "db_range": (-25.5, 3.0)}]


def libm_cases(planes_):
    """(label, scene, channels, stokes, films, spe, tm, s) over gamma / sRGB / dB, the three modes, the four plane counts and the film kinds.
    The colour tables are grey and turbo: a table multiplies the operator's error by its slope, (n - 1) x the largest step between neighbours —
    1 for grey, 12.4 for the 256-entry turbo table (its steepest channel), but up to n - 1 for a random table (measured with 64 random entries: 1.3e-5 = 63 x the
    operator's 2e-7, which says nothing about the operator).  Random tables are covered bit for bit by the libm-free test."""
    from wave_tracer_amd import imageio
    tables = [grey_table(), imageio.colour_table("turbo")]
    for sc, channels, stokes in planes_:
        for kind, spe in FILM_CASES:
            films = make_films(sc.height, sc.width, channels, stokes, 13, kind)
            for op in LIBM_OPS:
                for k, mode in enumerate(MODES):
                    tm = dict(op, mode=mode, table=tables[(k + stokes) % 2])
                    yield op["op"], sc, channels, stokes, films, spe, tm, stokes - 1


def test_gamma_srgb_db_against_the_f64_restatement(planes):
    """f32 output within 10 x the measured maximum difference (and below 1e-5); u8 / u16 within ONE code of the quantised restatement, every pixel;
    NaN where the restatement is NaN (code 0)."""
    worst = {}
    for op, sc, channels, stokes, (v, w, l), spe, tm, s in libm_cases(planes):
        want = restate(channels, stokes, v, w, l, spe, tm, s)
        got = sc.tonemap_host(v, w, l, spe, tm, s, threads=4)
        worst[op] = max(worst.get(op, 0.0), nan_equal_maxdiff(got, want))
        for fmt in ("u8", "u16"):
            q = sc.tonemap_host(v, w, l, spe, tm, s, fmt=fmt).astype(np.int64)
            assert np.abs(q - quantise(want, fmt)).max() <= 1, (op, tm["mode"], fmt)
            assert not q[np.isnan(want)].any()
    for op, m in sorted(worst.items()):
        check_measured(f"host/{op}", m)


def test_refused_calls_say_why(planes, tmp_path):
    from wave_tracer_amd import WtgpuError
    sc, channels, stokes = planes[0]
    v, w, l = make_films(sc.height, sc.width, channels, stokes, 1)
    with pytest.raises(WtgpuError, match=r"stokes_component 1 out of range \(the film has 1\)"):
        sc.tonemap_host(v, w, l, 1, {"op": "linear", "mode": "normal"}, 1)
    with pytest.raises(WtgpuError, match="'function' operator is not supported"):
        sc.tonemap_host(v, w, l, 1, {"op": "function", "mode": "normal"})
    with pytest.raises(WtgpuError, match='colour map "Magma" is not one the library tabulates .*pass a table'):
        sc.tonemap_host(v, w, l, 1)        # the bundled scene's default: linear / select through Magma
    with pytest.raises(WtgpuError, match="pass one"):
        sc.tonemap_host(v, w, l, 1, {"op": "linear", "mode": "select"})
    with pytest.raises(WtgpuError, match="2 .. 1024 RGB entries"):
        sc.tonemap_host(v, w, l, 1, {"op": "linear", "mode": "select", "table": random_table(1)})
    # a scene file's own spec: Turbo is tabulated by the library (the polynomial of imageio.colourmap), Magma is not; a function is refused
    from wave_tracer_amd import imageio
    turbo = _load(tmp_path, "t.xml", response=MONO, width=8, height=8,
                  tonemap='<tonemap type="dB"><range value="-60 .. 0"/><string name="colourmap" value="Turbo"/></tonemap>')
    fv, fw, fl = make_films(8, 8, 1, 1, 2)
    own = turbo.tonemap_host(fv, fw, fl, 3)
    explicit = turbo.tonemap_host(fv, fw, fl, 3, dict(turbo.tonemap_spec, table=imageio.colour_table("turbo")))
    assert nan_equal_maxdiff(own, explicit) < 1e-6 and np.nanmax(own) > 0
    fn = _load(tmp_path, "fn.xml", response=MONO, width=8, height=8, tonemap='<tonemap type="function"><function value="sqrt(value)"/></tonemap>')
    with pytest.raises(WtgpuError, match="'function' operator is not supported"):
        fn.tonemap_host(fv, fw, fl, 3)


def test_colour_table_samples_the_maps(built):
    from wave_tracer_amd import imageio
    g, t = imageio.colour_table("grey", 5), imageio.colour_table("turbo")
    assert g.dtype == F32 and np.array_equal(g[:, 0], F32([0, .25, .5, .75, 1])) and (g[:, 0:1] == g).all()
    assert t.shape == (256, 3) and np.allclose(t, imageio.colourmap(np.arange(256) / 255.0, "turbo"), atol=1e-7)
    with pytest.raises(ValueError):
        imageio.colour_table("magma")
