"""Line-of-sight maps (wtgpu_line_of_sight_host, csrc/wt/los.h) on the CPU: per sensor element — or caller's point — and selected emitter the
share of the samples that see the emitter and the means of distance, direction and cosine; per element the mean point, the number of emitters
seen and the nearest of them.  The host twin runs the header the device kernels run (tests/test_gpu_los.py compares them bit for bit).

The scene: a virtual-plane sensor in z = 0 facing +z, 37 x 23 elements of 0.1 m whose centres sit at odd multiples of 0.05 m; one horizontal
rectangle at z = 1 m over x, y in [0.5, 1.5] m; emitter 0 (A) a point at (1, 1, 2) above the rectangle, 1 (B) a point at (3, 1.2, 0.5) below
it, 2 (C) a point at (1, 1, -1) behind the sensor, 3 (D) directional, the direction to it (1, 0, 1) / sqrt 2.  The borders of the shadows are
multiples of 0.5 m, so no centre lies on one."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_sensor_mask import _write

W, H, EL = 37, 23, 0.1
NONE = 0xFFFFFFFF
EM_A, EM_B, EM_C = (1.0, 1.0, 2.0), (3.0, 1.2, 0.5), (1.0, 1.0, -1.0)
DIR_D = np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0)
MAPS = ("visible", "distance", "direction", "cos")
ELEM = ("point", "nearest_distance")
IDS = ("n_visible", "nearest")
ALL = dict(maps=MAPS, elem=ELEM, ids=IDS)


def los_xml(cx=1.05, cy=1.05):
    point = lambda p: (f'<emitter type="point"><point name="position" value="{p[0]}m, {p[1]}m, {p[2]}m"/>'
                       '<spectrum name="radiant_intensity" type="discrete" wavelength="1GHz" value="1"/></emitter>')
    return f'''<scene version="0.1.0">
  <integrator type="plt_path"><integer name="max_depth" value="4"/><string name="direction" value="forward"/></integrator>
  <sensor type="virtual_plane" id="coverage"><transform name="to_world"><translate x="{cx!r}m" y="{cy!r}m"/></transform>
    <quantity name="alpha" value=".001°"/><quantity name="extent" value="{W * EL!r} m, {H * EL!r} m"/>
    <film type="array"><integer name="width" value="{W}"/><integer name="height" value="{H}"/>
      <response type="monochromatic"><spectrum type="discrete" wavelength="1GHz"/></response></film></sensor>
  {point(EM_A)}{point(EM_B)}{point(EM_C)}
  <emitter type="directional"><transform name="to_world"><lookat target="0m,0m,0m" origin="1m,0m,1m" up="0,1,0"/></transform>
    <spectrum name="irradiance" type="discrete" wavelength="1GHz" value="1"/></emitter>
  <shape type="rectangle" id="occluder"><point name="p" x="0.5m" y="0.5m" z="1m"/><point name="x" x="1m" y="0m" z="0m"/>
    <point name="y" x="0m" y="1m" z="0m"/><bsdf type="twosided"><bsdf type="diffuse"><spectrum name="reflectance" constant=".5"/></bsdf></bsdf></shape>
</scene>'''


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same(x, y):
    return set(x) == set(y) and all(_same_bits(x[k], y[k]) for k in x)


def _within_ulps(got, want64, ulps=4):
    """|got - want| <= ulps x the f32 spacing at want, element by element"""
    return (np.abs(got.astype(np.float64) - want64) <= ulps * np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)).all()


@pytest.fixture(scope="module")
def plane(built, tmp_path_factory):
    from wave_tracer_amd import Scene
    sc = Scene.from_xml(_write(tmp_path_factory.mktemp("los"), "los.xml", los_xml()))
    assert (sc.width, sc.height) == (W, H) and sc.info.sensor_type == 1
    assert [e["type"] for e in sc.emitter_summary()] == ["point", "point", "point", "directional"]
    return sc


@pytest.fixture(scope="module")
def shifted(built, tmp_path_factory):
    """the same with the sensor moved by half an element: the centres lie ON the multiples of 0.1 m, every shadow border cuts a row of elements in two"""
    from wave_tracer_amd import Scene
    return Scene.from_xml(_write(tmp_path_factory.mktemp("los_shifted"), "los_shifted.xml", los_xml(1.0, 1.0)))


@pytest.fixture(scope="module")
def centres(plane):
    """the full query at the elements' centres, front_only on and off: shared, never changed"""
    return plane.line_of_sight_host(samples=0, **ALL), plane.line_of_sight_host(samples=0, front_only=False, **ALL)


def _expected_visible(p):
    """the closed form at points p [..., 3] in z = 0, with FRONT_ONLY: [..., 4] bool"""
    x, y = p[..., 0], p[..., 1]
    a = ~((x > 0) & (x < 2) & (y > 0) & (y < 2))
    d = ~((x > -0.5) & (x < 0.5) & (y > 0.5) & (y < 1.5))
    return np.stack([a, np.ones_like(a), np.zeros_like(a), d], axis=-1)


def test_closed_form_at_the_centres(plane, centres):
    r, back = centres
    assert set(r) == set(MAPS + ELEM + IDS)
    assert all(r[k].shape == (H, W, 4) and r[k].dtype == np.float32 for k in ("visible", "distance", "cos")) and r["direction"].shape == (H, W, 4, 3)
    assert r["point"].shape == (H, W, 3) and r["nearest_distance"].shape == (H, W) and all(r[k].shape == (H, W) and r[k].dtype == np.uint32 for k in IDS)
    p = r["point"].astype(np.float64)
    # the centres: odd multiples of 0.05 m in z = 0, to the rounding of the f32 sums that place them
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    assert np.abs(p[..., 0] - (-0.75 + 0.1 * i)).max() < 1e-6 and np.abs(p[..., 1] - (-0.05 + 0.1 * j)).max() < 1e-6 and not p[..., 2].any()
    want = _expected_visible(p)
    assert want[..., 0].sum() == H * W - 400 and (~want[..., 3]).sum() == 100      # 20 x 20 centres in A's shadow, 10 x 10 in D's
    assert np.array_equal(r["visible"], want.astype(np.float32))
    # without FRONT_ONLY the emitter behind the sensor is seen from everywhere, and nothing else changes
    want_back = want.copy()
    want_back[..., 2] = True
    assert np.array_equal(back["visible"], want_back.astype(np.float32))
    for k in ("distance", "direction", "cos", "point"):
        assert _same_bits(r[k], back[k]), k
    # distance, direction and cosine against f64 from the same points (the sensor's normal is +z), whether the emitter is visible or not
    for e, pos in enumerate((EM_A, EM_B, EM_C)):
        v = np.asarray(pos, dtype=np.float32).astype(np.float64) - p          # (the scene holds the positions in f32: 1.2 is not 1.2f)
        dist = np.linalg.norm(v, axis=-1)
        assert _within_ulps(r["distance"][..., e], dist), e
        assert _within_ulps(r["direction"][..., e, :], v / dist[..., None]), e
        assert _within_ulps(r["cos"][..., e], v[..., 2] / dist), e
    assert not r["distance"][..., 3].any()
    assert _within_ulps(r["direction"][..., 3, :], np.broadcast_to(DIR_D, (H, W, 3)), 1) and _within_ulps(r["cos"][..., 3], np.full((H, W), DIR_D[2]), 1)
    # the ids, restated: the directional emitter counts with distance 0, so it is the nearest wherever it is seen
    for q, vis in ((r, want), (back, want_back)):
        assert np.array_equal(q["n_visible"], vis.sum(axis=-1).astype(np.uint32))
        d = np.where(vis, q["distance"], np.float32(np.inf))
        assert np.array_equal(q["nearest"], np.argmin(d, axis=-1).astype(np.uint32))           # (B is seen everywhere: there is always one)
        assert np.array_equal(q["nearest_distance"], d.min(axis=-1))
    assert (r["nearest"][want[..., 3]] == 3).all() and (r["nearest"][~want[..., 3]] < 2).all()


def test_ties_and_none_by_hand(plane, centres):
    """Caller points: a point at z = 0.5 is as far from A (z = 2) as from C (z = -1), bit for bit — the first of the selection wins; an element
    in A's shadow that selects A and the emitter behind it sees none."""
    pts = np.ascontiguousarray(centres[0]["point"]).copy()
    pts[0, 0] = (5.0, 5.0, 0.5)
    kw = dict(points=pts, front_only=False, maps=("visible", "distance"), elem=("nearest_distance",), ids=IDS)
    ac, ca = plane.line_of_sight_host(emitters=[0, 2], **kw), plane.line_of_sight_host(emitters=[2, 0], **kw)
    for q in (ac, ca):
        assert q["visible"][0, 0].tolist() == [1, 1] and q["distance"][0, 0, 0] == q["distance"][0, 0, 1] == q["nearest_distance"][0, 0]
        assert q["n_visible"][0, 0] == 2 and q["nearest"][0, 0] == 0
    # every other point is in z = 0, where C (1 m behind) is nearer than A (2 m above) by more than rounding
    assert (ac["nearest"].ravel()[1:] == 1).all() and (ca["nearest"].ravel()[1:] == 0).all()
    none = plane.line_of_sight_host(emitters=[0, 2], maps=("visible",), elem=("nearest_distance",), ids=IDS)
    shadow = ~_expected_visible(centres[0]["point"].astype(np.float64))[..., 0]
    assert shadow.sum() == 400
    assert (none["n_visible"][shadow] == 0).all() and (none["nearest"][shadow] == NONE).all() and not none["nearest_distance"][shadow].any()
    assert (none["n_visible"][~shadow] == 1).all() and (none["nearest"][~shadow] == 0).all() and (none["nearest_distance"][~shadow] > 2).all()


@pytest.mark.parametrize("samples", [1, 7, 32])
def test_samples_layout_and_equivalences(plane, shifted, centres, samples):
    r = plane.line_of_sight_host(samples=samples, seed=5, **ALL)
    # the points stay in their elements, and no element of this sensor straddles a shadow border: every sample sees what the centre sees
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    p = r["point"].astype(np.float64)
    assert (np.abs(p[..., 0] - (-0.75 + 0.1 * i)) <= 0.05 + 1e-6).all() and (np.abs(p[..., 1] - (-0.05 + 0.1 * j)) <= 0.05 + 1e-6).all()
    assert not p[..., 2].any() and not _same_bits(r["point"], centres[0]["point"])
    assert np.array_equal(r["visible"], centres[0]["visible"]) and np.array_equal(r["nearest"], centres[0]["nearest"])
    assert np.abs(r["distance"].astype(np.float64) - centres[0]["distance"]).max() < 0.08 and not _same_bits(r["distance"], centres[0]["distance"])
    # moved by half an element, the borders cut elements in two: shares j / samples, strictly between 0 and 1 only in the rows and columns of a border
    s = shifted.line_of_sight_host(samples=samples, seed=5, **ALL)
    assert np.array_equal(s["visible"] * samples, np.round(s["visible"] * samples)) and s["visible"].min() == 0 and s["visible"].max() == 1
    assert np.array_equal(s["visible"][..., 1:3], np.broadcast_to(np.float32([1, 0]), (H, W, 2)))
    c = shifted.line_of_sight_host(samples=0, maps=(), elem=("point",), ids=())["point"].astype(np.float64)
    for e, (xs, ys) in ((0, ((0, 2), (0, 2))), (3, ((-0.5, 0.5), (0.5, 1.5)))):
        part = (s["visible"][..., e] > 0) & (s["visible"][..., e] < 1)
        on_border = np.minimum.reduce([np.abs(c[..., 0] - x) for x in xs] + [np.abs(c[..., 1] - y) for y in ys]) < 1e-6
        assert not (part & ~on_border).any() and (part.any() == (samples > 1)), e
    assert np.array_equal(s["n_visible"], (s["visible"] > 0).sum(axis=-1).astype(np.uint32))
    assert np.array_equal(r["n_visible"], (r["visible"] > 0).sum(axis=-1).astype(np.uint32))
    # thread counts, seeds
    for threads in (1, 5):
        assert _same(plane.line_of_sight_host(samples=samples, seed=5, threads=threads, **ALL), r), threads
    other = plane.line_of_sight_host(samples=samples, seed=6, **ALL)
    assert not _same_bits(other["point"], r["point"]) and not _same_bits(other["distance"], r["distance"])
    # a selection of one emitter, and of two in another order, are the slices of the full call
    for sel in ([0], [3], [2, 0]):
        q = plane.line_of_sight_host(samples=samples, seed=5, emitters=sel, maps=MAPS, elem=("point",), ids=())
        for k in MAPS:
            assert _same_bits(q[k], np.ascontiguousarray(r[k][:, :, sel])), (sel, k)
        assert _same_bits(q["point"], r["point"])


def test_every_subset_of_the_bits_is_a_slice_of_the_full_query(plane):
    full = plane.line_of_sight_host(samples=7, seed=2, **ALL)
    subsets = lambda names: [c for n in range(len(names) + 1) for c in itertools.combinations(names, n)]
    n = 0
    for maps in subsets(MAPS):
        # every subset of the pair maps with every subset of the element groups, turn by turn (16 x 4 calls, not 16 x 16)
        for elem, ids in zip(subsets(ELEM), subsets(IDS)[::-1]):
            if not (maps or elem or ids):
                continue
            q = plane.line_of_sight_host(samples=7, seed=2, maps=maps, elem=elem, ids=ids)
            assert set(q) == set(maps + elem + ids)
            for k in q:
                assert _same_bits(np.ascontiguousarray(q[k]), np.ascontiguousarray(full[k])), (maps, elem, ids, k)
            n += 1
    assert n == 64
    for elem, ids in itertools.product(subsets(ELEM), subsets(IDS)):
        if elem or ids:
            q = plane.line_of_sight_host(samples=7, seed=2, maps=(), elem=elem, ids=ids)
            assert all(_same_bits(np.ascontiguousarray(q[k]), np.ascontiguousarray(full[k])) for k in q) and set(q) == set(elem + ids)


def test_mask_and_nan_points_pass_through(plane, centres):
    r = centres[0]
    mask = np.ones((H, W), np.float32)
    mask[3:9, 4:30] = 0
    mask[10, 10], mask[11, 11] = -1, np.nan
    out = ~(mask > 0)
    for samples in (0, 7):
        full = plane.line_of_sight_host(samples=samples, seed=5, **ALL)
        q = plane.line_of_sight_host(samples=samples, seed=5, mask=mask, **ALL)
        for k in MAPS + ELEM:
            assert not q[k][out].any() and _same_bits(q[k][~out], full[k][~out]), k
        assert not q["n_visible"][out].any() and (q["nearest"][out] == NONE).all()
        assert all(np.array_equal(q[k][~out], full[k][~out]) for k in IDS)
    # a point that is not finite: the same zeros; its neighbours are untouched
    pts = np.ascontiguousarray(r["point"]).copy()
    nrm = np.broadcast_to(np.float32([0, 0, 1]), (H, W, 3)).copy()
    pts[2, 3, 1], pts[5, 6, 0], pts[7, 7, 2] = np.nan, np.inf, -np.inf
    bad = ~np.isfinite(pts).all(axis=-1)
    q = plane.line_of_sight_host(points=pts, normals=nrm, **ALL)
    for k in MAPS + ELEM:
        assert not q[k][bad].any() and _same_bits(q[k][~bad], r[k][~bad]), k
    assert not q["n_visible"][bad].any() and (q["nearest"][bad] == NONE).all() and np.array_equal(q["nearest"][~bad], r["nearest"][~bad])


def test_caller_points_equal_the_sensors_own(plane, centres):
    r, back = centres
    pts = np.ascontiguousarray(r["point"])
    nrm = np.broadcast_to(np.float32([0, 0, 1]), (H, W, 3)).copy()
    assert _same(plane.line_of_sight_host(points=pts, normals=nrm, **ALL), r)
    assert _same(plane.line_of_sight_host(points=pts, normals=nrm, front_only=False, **ALL), back)
    # without normals: no cosine, no front side; the rest is the same
    q = plane.line_of_sight_host(points=pts, front_only=False, maps=("visible", "distance", "direction"), elem=ELEM, ids=IDS)
    assert all(_same_bits(np.ascontiguousarray(q[k]), np.ascontiguousarray(back[k])) for k in q) and "cos" not in q
    # t_min: a range that starts beyond the occluder (1 m above the sensor, at most sqrt 2 m along a ray to A from its shadow) does not see it
    far = plane.line_of_sight_host(points=pts, normals=nrm, t_min=1.5, emitters=[0], maps=("visible",), ids=())
    assert (far["visible"] == 1).all()


def test_t_min_on_first_hit_positions(built):
    """cornell_box from its camera: the first-hit positions lie ON the surfaces (to rounding), so with t_min = 0 some of them shadow themselves;
    render.shadow_guides' default t_min (1e-4 diagonals) does not start inside the surface.  Only that the two differ, and that the default
    sees a lamp from the floor, is asserted."""
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import SHADOW_GUIDE_T_MIN, shadow_guides
    sc = Scene("cornell_box", res=32, mesh_detail=0)
    kinds = [e["type"] for e in sc.emitter_summary()]
    E = sum(k != "area" for k in kinds)
    assert "area" in kinds and E >= 1
    guide, scales, ids = shadow_guides(sc, host=True)
    assert guide.shape == (sc.height, sc.width, E) and guide.dtype == np.float32 and scales == [pytest.approx(2.7777777)] * E and ids is None
    assert np.isin(guide, (0, 1)).all()
    fh = sc.first_hit_host(samples=0, maps=("coverage", "position", "normal_geo"), ids=())
    kw = dict(points=fh["position"], normals=fh["normal_geo"], mask=fh["coverage"], front_only=False, maps=("visible",), ids=())
    st = sc.stats()
    t_min = SHADOW_GUIDE_T_MIN * float(np.linalg.norm(np.subtract(st["world_max"], st["world_min"])))
    assert t_min > 0 and _same_bits(sc.line_of_sight_host(t_min=t_min, **kw)["visible"], guide)
    zero = sc.line_of_sight_host(t_min=0.0, **kw)["visible"]
    assert not np.array_equal(zero, guide)
    floor = (fh["coverage"] > 0) & (fh["normal_geo"][..., 1] > 0.99)
    assert floor.any() and guide[floor].max() == 1
    assert not guide[fh["coverage"] == 0].any()
    # an area emitter is refused by name, and leaves the default selection
    from wave_tracer_amd import WtgpuError
    with pytest.raises(WtgpuError, match=f"emitter {kinds.index('area')} is an area emitter"):
        sc.line_of_sight_host(emitters=[kinds.index("area")], **kw)
    with pytest.raises(WtgpuError, match="not one"):
        sc.line_of_sight_host()                                   # a perspective sensor without points


def test_refusals(plane, centres):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import LosSpec, _check, load_library
    lib = load_library()
    pts = np.ascontiguousarray(centres[0]["point"])
    maps, elem, ids = np.zeros((H, W, 4, 6), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W, 2), np.uint32)

    def call(spec, points=None, normals=None, m=maps, e=elem, i=ids):
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(lib.wtgpu_line_of_sight_host(plane._h, C.byref(spec), ptr(points), ptr(normals), None, 1, ptr(m), ptr(e), ptr(i)))

    def spec(samples=0, maps=15, elem=3, ids=3, flags=1, emitters=(), t_min=0.0):
        return LosSpec(samples, maps, elem, ids, flags, len(emitters), (C.c_uint32 * 32)(*emitters[:32]), t_min, 0, 1)

    call(spec())                                                  # (the full query is fine)
    for s, kw, msg in ((spec(samples=1), dict(points=pts), "caller points take samples = 0"),
                       (spec(samples=4097), {}, "0 .. 4096 samples"),
                       (spec(maps=16), {}, "unknown map bits"), (spec(elem=4), {}, "unknown element bits"), (spec(ids=4), {}, "unknown id bits"),
                       (spec(flags=2), {}, "unknown flag bits"),
                       (spec(maps=0, elem=0, ids=0), {}, "nothing requested"),
                       (spec(), dict(m=None), "maps pointer is NULL"), (spec(), dict(e=None), "elem pointer is NULL"), (spec(), dict(i=None), "ids pointer is NULL"),
                       (spec(flags=0), dict(points=pts), "COS needs a normal"), (spec(maps=7), dict(points=pts), "FRONT_ONLY needs a normal"),
                       (spec(t_min=-1.0), {}, "t_min"), (spec(t_min=float("nan")), {}, "t_min"), (spec(t_min=float("inf")), {}, "t_min"),
                       (spec(emitters=(4,)), {}, "emitter index 4 out of range"), (spec(emitters=(1, 3, 1)), {}, "emitter 1 is selected twice")):
        with pytest.raises(WtgpuError, match=msg):
            call(s, **kw)
    many = spec()
    many.n_emitters = 33
    with pytest.raises(WtgpuError, match="at most 32 emitters"):
        call(many)
    # a requested group may not be NULL, a group that is not requested may
    call(spec(maps=1, elem=0, ids=0), e=None, i=None)
    # the Python layer names what it does not know, and the sizes it expects
    with pytest.raises(ValueError, match="unknown map 'depth'"):
        plane.line_of_sight_host(maps=("depth",))
    with pytest.raises(ValueError, match="points"):
        plane.line_of_sight_host(points=np.zeros((3, 3, 3), np.float32))
    with pytest.raises(ValueError, match="emitter indices"):
        plane.line_of_sight_host(emitters=[])
    with pytest.raises(WtgpuError, match="upload"):
        plane.line_of_sight()


def test_empty_selection_is_refused(built):
    from wave_tracer_amd import Scene, WtgpuError
    sc = Scene("furnace", res=8)
    assert all(e["type"] == "area" for e in sc.emitter_summary())
    with pytest.raises(WtgpuError, match="empty selection"):
        sc.line_of_sight_host(points=np.zeros((sc.height, sc.width, 3), np.float32), front_only=False)


def test_python_helpers(plane, shifted):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.render import los_masks, shadow_guides
    want = _expected_visible(plane.line_of_sight_host(maps=(), elem=("point",), ids=())["point"].astype(np.float64))
    for emitter in (None, 0, 2, 3):
        for samples in (0, 7):
            los, nlos = los_masks(plane, emitter=emitter, samples=samples, host=True)
            assert los.shape == nlos.shape == (H, W) and los.dtype == nlos.dtype == np.float32 and np.isin(los, (0, 1)).all()
            assert los.sum() + nlos.sum() == H * W and np.array_equal(los + nlos, np.ones((H, W), np.float32))
            if samples == 0:
                assert np.array_equal(los == 1, np.ones((H, W), bool) if emitter is None else want[..., emitter])
    # samples at a border: an element counts as in sight as soon as one of its samples is
    share = shifted.line_of_sight_host(samples=7, seed=1, emitters=[0], maps=("visible",), ids=())["visible"][..., 0]
    assert np.array_equal(los_masks(shifted, emitter=0, samples=7, host=True)[0] == 1, share > 0) and (share > 0).sum() > (share == 1).sum()
    with pytest.raises(WtgpuError, match="perspective sensor"):
        shadow_guides(plane, host=True)                         # first_hit's own refusal
    with pytest.raises(WtgpuError, match="upload"):
        los_masks(plane)
