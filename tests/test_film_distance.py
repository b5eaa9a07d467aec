"""Exact Euclidean distance transform of a label plane with the nearest site (wt/film_distance.h: wtgpu_film_distance_host; render.distance, dilate,
erode, opening, closing, nearest_segment, zones_from_distance) on the CPU: the host twin against a brute force written here — for every pixel the
minimum over all sites of (d², index), in numpy int64; it calls nothing of the library — and, where scipy imports, against
scipy.ndimage.distance_transform_edt.  tests/test_gpu_film_distance.py runs the device kernels against the host twin on the same shapes and plans.

There is no tolerance anywhere: squared pixel distances are integers and ties go to the smaller pixel index, so both planes and every field of
the info must be equal."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_film_segments import SHAPES, segments_scene
from test_film_stats import F32, SPE, stats_films, stats_scene, restate_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
assert SHAPES == [(37, 23), (130, 67), (256, 192), (257, 256), (4096, 1), (1, 4096)]
LARGE = SHAPES[2:4]          # the brute force runs there only on plans of at most MAX_BRUTE_SITES sites
MAX_BRUTE_SITES = 2048
PLANS = ("all", "none", "corners_centre", "row_first", "row_last", "column", "diagonal", "checker", "perc001", "perc05", "random5", "checker_mask", "mask_none")
INFO = ("n_sites", "max_dist2", "argmax")


def cases():
    """every plan at every shape"""
    return [(w, h, plan) for w, h in SHAPES for plan in PLANS]


# ---- plans ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan(name, height, width):
    rng = np.random.default_rng(len(name) * 1000 + height + width)
    yy, xx = np.mgrid[0:height, 0:width]
    classes, mask = None, None
    if name == "none":
        classes = np.full((height, width), NONE)
    elif name == "corners_centre":
        classes = np.full((height, width), NONE)
        for y, x in ((0, 0), (0, width - 1), (height - 1, 0), (height - 1, width - 1), (height // 2, width // 2)):
            classes[y, x] = 2
    elif name == "row_first":
        classes = np.where(yy == 0, 1, NONE)
    elif name == "row_last":
        classes = np.where(yy == height - 1, 1, NONE)
    elif name == "column":
        classes = np.where(xx == width // 3, 1, NONE)
    elif name == "diagonal":
        classes = np.where(yy * max(width - 1, 1) == xx * max(height - 1, 1), 4, NONE) if min(width, height) > 1 else np.where(yy + xx == 7, 4, NONE)
    elif name == "checker":
        classes = np.where((yy + xx) % 2 == 0, 3, NONE)
    elif name.startswith("perc"):       # seeded site percolation at p = 0.01 and 0.5
        classes = np.where(np.random.default_rng(7 + len(name)).random((height, width)) < {"perc001": 0.01, "perc05": 0.5}[name], 1, NONE)
    elif name in ("random5", "checker_mask", "mask_none"):
        classes = np.where(rng.random((height, width)) < 0.1, NONE, rng.integers(0, 5, (height, width)))
    elif name != "all":
        raise KeyError(name)
    if name == "checker_mask":          # the segments tests' mask — excluded: zeros, negatives, -0 and a NaN
        mask = np.where((yy // 3 + xx // 2) % 2 == 0, 0.5, rng.choice(np.array([0.0, -1.0, -0.0], F32), (height, width))).astype(F32)
        mask[height // 2, width // 2] = np.nan
    if name == "mask_none":
        mask = np.zeros((height, width), F32)
        mask[0, 0] = np.nan
    if classes is not None:
        classes = np.ascontiguousarray(classes.astype(np.uint32))
        classes.setflags(write=False)
    if mask is not None:
        mask.setflags(write=False)
    return classes, mask


def plan(name, height, width):
    """(classes uint32 [height, width] or None, mask float32 or None); shared between the tests, read-only"""
    return _plan(name, height, width)


def sites_of(classes, mask, invert, height, width):
    """the bool plane of the sites, restated: a member has mask > 0 (a NaN has not) and a class other than 0xFFFFFFFF"""
    member = np.ones((height, width), bool) if classes is None else classes != NONE
    if mask is not None:
        member = member & (mask > 0)
    return member != bool(invert)


# ---- the brute force ----------------------------------------------------------------------------------------------------------------------------
def brute_force(sites):
    """For every pixel the minimum over all sites of (d², index) as one int64 key d² 2^32 + index -> dist2, nearest (uint32), the info."""
    height, width = sites.shape
    n = height * width
    sy, sx = np.nonzero(sites)
    s_index = (sy * width + sx).astype(np.int64)
    if s_index.size == 0:
        return {"dist2": np.full((height, width), NONE, np.uint32), "nearest": np.full((height, width), NONE, np.uint32), "n_sites": 0, "max_dist2": NONE, "argmax": 0}
    key = np.empty(n, np.int64)
    step = max(1, (1 << 22) // s_index.size)
    for p0 in range(0, n, step):
        p = np.arange(p0, min(p0 + step, n), dtype=np.int64)
        d2 = (p[:, None] % width - sx[None, :]) ** 2 + (p[:, None] // width - sy[None, :]) ** 2
        key[p0:p0 + step] = (d2 * (1 << 32) + s_index[None, :]).min(axis=1)
    dist2 = (key >> 32).astype(np.uint32).reshape(height, width)
    return {"dist2": dist2, "nearest": (key & 0xFFFFFFFF).astype(np.uint32).reshape(height, width), "n_sites": int(s_index.size), "max_dist2": int(dist2.max()),
            "argmax": int(np.argmax(dist2))}


@functools.lru_cache(maxsize=None)
def _want(name, height, width, invert):
    sites = sites_of(*plan(name, height, width), invert, height, width)
    if (width, height) in LARGE and sites.sum() > MAX_BRUTE_SITES:
        return None
    out = brute_force(sites)
    for k in ("dist2", "nearest"):
        out[k].setflags(write=False)
    return out


def same_result(got, want, label):
    """every field of the info and both planes (as uint32 bits) are equal"""
    for k in INFO:
        assert got[k] == want[k], (label, k, got[k], want[k])
    for k in ("dist2", "nearest"):
        a, b = got[k], want[k]
        if a is None or b is None:
            assert a is None and b is None, (label, k)
            continue
        a, b = np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (label, k, np.argwhere(a != b)[:4].tolist())


def info_from_numpy(got, sites, label):
    dist2 = got["dist2"]
    assert (got["n_sites"], got["max_dist2"], got["argmax"]) == (int(sites.sum()), int(dist2.max()), int(np.argmax(dist2))), label


def consistent(got, sites, label):
    """What holds of a right answer without the brute force: dist2 is 0 exactly on the sites; nearest is a site, at exactly dist2; and no site
    with a smaller index is equally far along the row and the column through the pixel."""
    height, width = sites.shape
    dist2, near = got["dist2"].astype(np.int64), got["nearest"].astype(np.int64)
    yy, xx = np.mgrid[0:height, 0:width]
    assert np.array_equal(dist2 == 0, sites), label
    assert (near < height * width).all() and sites.reshape(-1)[near].all(), label
    ny, nx = near // width, near % width
    assert np.array_equal((nx - xx) ** 2 + (ny - yy) ** 2, dist2), label
    for along_row in (True, False):
        line = sites if along_row else sites.T                   # [lines, positions along the line]
        for n_line in range(line.shape[0]):
            s = np.nonzero(line[n_line])[0]
            if s.size == 0:
                continue
            d2 = (np.arange(line.shape[1])[:, None] - s[None, :]) ** 2                    # [positions, sites of the line]
            index = (n_line * width + s) if along_row else (s * width + n_line)
            key = (d2 * (1 << 32) + index[None, :]).min(axis=1)
            mine = (dist2[n_line] if along_row else dist2[:, n_line]) * (1 << 32) + (near[n_line] if along_row else near[:, n_line])
            assert (mine <= key).all(), (label, along_row, n_line)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_distance")
    return {(w, h): segments_scene(d, w, h) for w, h in SHAPES}


@pytest.mark.parametrize("width,height,name", cases())
def test_host_twin_equals_the_brute_force(scenes, width, height, name):
    sc = scenes[(width, height)]
    classes, mask = plan(name, height, width)
    for invert in (False, True):
        got = sc.film_distance_host(classes, mask=mask, invert=invert, nearest=True, threads=4)
        assert got["dist2"].dtype == np.uint32 and got["nearest"].dtype == np.uint32
        sites = sites_of(classes, mask, invert, height, width)
        info_from_numpy(got, sites, (name, invert))
        want = _want(name, height, width, invert)
        if want is not None:
            same_result(got, want, (name, invert))
            continue
        # a dense plan at a large shape
        consistent(got, sites, (name, invert))
        try:
            from scipy import ndimage
        except ImportError:
            continue
        edt = ndimage.distance_transform_edt(~sites)
        assert np.array_equal(np.rint(edt * edt).astype(np.int64), got["dist2"].astype(np.int64)), (name, invert)


def test_the_large_shapes_meet_both_kinds_of_check():
    """at 256 x 192 and 257 x 256 some plans go to the brute force and the dense ones to scipy and the consistency check"""
    for width, height in LARGE:
        kinds = {_want(name, height, width, invert) is None for name in PLANS for invert in (False, True)}
        assert kinds == {True, False}
        assert _want("perc001", height, width, False) is not None and _want("perc05", height, width, False) is None


def test_what_the_plans_are_known_to_give(scenes):
    for width, height in SHAPES[:2]:
        sc = scenes[(width, height)]
        n = width * height
        k = lambda name, **kw: sc.film_distance_host(plan(name, height, width)[0], mask=plan(name, height, width)[1], nearest=True, **kw)
        every = k("all")
        assert (every["n_sites"], every["max_dist2"], every["argmax"]) == (n, 0, 0) and not every["dist2"].any()
        assert np.array_equal(every["nearest"].reshape(-1), np.arange(n, dtype=np.uint32))
        for got in (k("none"), k("mask_none"), k("all", invert=True)):
            assert (got["n_sites"], got["max_dist2"], got["argmax"]) == (0, NONE, 0) and (got["dist2"] == NONE).all() and (got["nearest"] == NONE).all()
        yy, xx = np.mgrid[0:height, 0:width]
        first, last = k("row_first"), k("row_last")
        assert np.array_equal(first["dist2"], yy ** 2) and np.array_equal(first["nearest"], xx) and first["argmax"] == (height - 1) * width
        assert np.array_equal(last["dist2"], (height - 1 - yy) ** 2) and np.array_equal(last["nearest"], (height - 1) * width + xx) and last["argmax"] == 0
        column = k("column")
        assert np.array_equal(column["dist2"], (xx - width // 3) ** 2) and np.array_equal(column["nearest"], yy * width + width // 3)
        assert column["n_sites"] == height and column["argmax"] == width - 1
        # without nearest the plane is not made
        assert sc.film_distance_host(None)["nearest"] is None


def _hand(sc, sites_xy, invert=False):
    """the transform of a plane whose sites are the given (x, y) — with invert the plane says so the other way round"""
    classes = np.full((sc.height, sc.width), 0 if invert else NONE, np.uint32)
    for x, y in sites_xy:
        classes[y, x] = NONE if invert else 6
    return sc.film_distance_host(classes, invert=invert, nearest=True, threads=1)


def test_ties_go_to_the_smaller_index(scenes):
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    at = lambda x, y: y * width + x
    for invert in (False, True):
        # left and right equally far: the left wins
        got = _hand(sc, [(10, 5), (14, 5)], invert)
        assert (got["dist2"][5, 12], got["nearest"][5, 12]) == (4, at(10, 5))
        # above and below: the upper wins
        got = _hand(sc, [(12, 3), (12, 7)], invert)
        assert (got["dist2"][5, 12], got["nearest"][5, 12]) == (4, at(12, 3))
        assert (got["dist2"][5, 0], got["nearest"][5, 0]) == (148, at(12, 3))
        # four sites at d² = 25 around (10, 8), at offsets (3, 4), (5, 0), (4, 3), (0, 5): the winner by index lies in the origin's row, in the LARGEST
        # column of the four — not in the smallest, which an outward search over the columns meets first
        ox, oy = 10, 8
        got = _hand(sc, [(ox + 3, oy + 4), (ox + 5, oy), (ox + 4, oy + 3), (ox, oy + 5)], invert)
        assert (got["dist2"][oy, ox], got["nearest"][oy, ox]) == (25, at(ox + 5, oy))
        same_result(got, brute_force(sites_of(None, None, False, height, width) & np.isin(np.arange(width * height).reshape(height, width),
                                                                                          [at(ox + 3, oy + 4), at(ox + 5, oy), at(ox + 4, oy + 3), at(ox, oy + 5)])), "four")
        # mirrored to the left and upwards the winner is the topmost: (ox, oy - 5), the column of the origin itself
        got = _hand(sc, [(ox - 3, oy - 4), (ox - 5, oy), (ox - 4, oy - 3), (ox, oy - 5)], invert)
        assert (got["dist2"][oy, ox], got["nearest"][oy, ox]) == (25, at(ox, oy - 5))
        # the sites (2, 0) and (0, 2) seen from (2, 2)
        got = _hand(sc, [(2, 0), (0, 2)], invert)
        assert (got["dist2"][2, 2], got["nearest"][2, 2]) == (4, at(2, 0))
        assert (got["dist2"][0, 0], got["nearest"][0, 0]) == (4, at(2, 0))


def test_the_result_does_not_depend_on_the_threads(scenes):
    width, height = SHAPES[1]
    sc = scenes[(width, height)]
    for name in ("perc001", "random5", "checker_mask", "corners_centre"):
        classes, mask = plan(name, height, width)
        for invert in (False, True):
            a = sc.film_distance_host(classes, mask=mask, invert=invert, nearest=True, threads=1)
            b = sc.film_distance_host(classes, mask=mask, invert=invert, nearest=True, threads=5)
            same_result(a, b, (name, invert))
            same_result(sc.film_distance_host(classes, mask=mask, invert=invert, threads=5), dict(a, nearest=None), (name, invert, "no nearest"))


def test_int32_bits_are_taken_like_uint32(scenes):
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    classes, _ = plan("random5", height, width)
    same_result(sc.film_distance_host(classes.view(np.int32), nearest=True), sc.film_distance_host(classes, nearest=True), "int32")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_say_why(scenes):
    import ctypes as C
    from wave_tracer_amd.api import FilmDistanceInfo, FilmDistanceSpec, load_library
    lib = load_library()
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    dist2 = np.full((height, width), 5, np.uint32)
    near = np.full((height, width), 6, np.uint32)
    info = FilmDistanceInfo(9, 9, 9, 0)

    def refused(spec, dist2_, info_, message):
        rc = lib.wtgpu_film_distance_host(sc.handle, C.byref(spec), None, None, 1, dist2_, near.ctypes.data, info_)
        assert (rc, lib.wtgpu_last_error().decode()) == (1, message)
        # the device entry point refuses the same things first, before it asks for an upload
        rc = lib.wtgpu_film_distance_device(sc.handle, None, C.byref(spec), None, None, dist2_, near.ctypes.data, info_)
        assert (rc, lib.wtgpu_last_error().decode()) == (1, message)
    ok = FilmDistanceSpec(0)
    refused(ok, None, C.byref(info), "film_distance: dist2 and info expected (one of them is NULL)")
    refused(ok, dist2.ctypes.data, None, "film_distance: dist2 and info expected (one of them is NULL)")
    for flags in (2, 3, 0x80000000):
        refused(FilmDistanceSpec(flags), dist2.ctypes.data, C.byref(info), f"film_distance: flags 0 or 1 (INVERT) expected, got {flags}")
    # the device call without an upload
    rc = lib.wtgpu_film_distance_device(sc.handle, None, C.byref(ok), None, None, dist2.ctypes.data, near.ctypes.data, C.byref(info))
    assert (rc, lib.wtgpu_last_error().decode()) == (1, "film_distance: scene not uploaded")
    assert (dist2 == 5).all() and (near == 6).all() and (info.n_sites, info.argmax, info.max_dist2) == (9, 9, 9)      # nothing was written
    # nearest may be NULL
    rc = lib.wtgpu_film_distance_host(sc.handle, C.byref(FilmDistanceSpec(1)), None, None, 1, dist2.ctypes.data, None, C.byref(info))
    assert rc == 0 and (info.n_sites, info.argmax, info.max_dist2) == (0, 0, NONE) and (dist2 == NONE).all() and (near == 6).all()


def test_a_sensor_wider_or_higher_than_32768_is_refused(built, tmp_path):
    """A scene holds nothing per pixel and the entry point refuses before it reads a plane: 65536 x 32768 is too wide, 32768 x 32769 too high;
    32768 x 32768 passes this check, and the next refusal in line answers."""
    import ctypes as C
    from wave_tracer_amd.api import FilmDistanceInfo, FilmDistanceSpec, load_library
    lib = load_library()
    dummy, info = np.zeros(16, np.uint32), FilmDistanceInfo()
    size = "film_distance: a sensor wider or higher than 32768 pixels (squared distances stay below 2^31 and a vertical offset fits 16 bits)"
    for width, height, message in ((65536, 32768, size), (32768, 32769, size), (32768, 32768, "film_distance: scene not uploaded")):
        sc = stats_scene(tmp_path, 1, width, height)
        spec = FilmDistanceSpec(0)
        if message == size:
            assert lib.wtgpu_film_distance_host(sc.handle, C.byref(spec), None, None, 1, dummy.ctypes.data, None, C.byref(info)) == 1
            assert lib.wtgpu_last_error().decode() == message
        assert lib.wtgpu_film_distance_device(sc.handle, None, C.byref(spec), None, None, dummy.ctypes.data, None, C.byref(info)) == 1
        assert lib.wtgpu_last_error().decode() == message
    assert not dummy.any()


def test_planes_of_another_kind_are_refused_in_python(scenes):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.render import dilate, erode, zones_from_distance
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    z = np.zeros((height, width), np.uint32)
    for bad in (z.astype(np.int64), z.astype(np.float32), z[:, :-1], z.T, np.zeros((width, height), np.uint32).T, z.tolist()):
        with pytest.raises(ValueError, match="film_distance_host: classes: a contiguous int32 or uint32 array"):
            sc.film_distance_host(bad)
    m = np.ones((height, width), F32)
    for bad in (m.astype(np.float64), m[:-1], np.ones((width, height), F32).T):
        with pytest.raises(ValueError, match="film_distance_host: mask: a contiguous float32 array"):
            sc.film_distance_host(z, mask=bad)
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_distance_device(None)
    with pytest.raises(ValueError, match="dilate: a bool plane expected"):
        dilate(sc, z, 1)
    with pytest.raises(ValueError, match="erode: a finite radius >= 0 expected"):
        erode(sc, z == 0, -1)
    with pytest.raises(ValueError, match="zones_from_distance: at least two"):
        zones_from_distance(z, [3, 3])


# ---- the helpers --------------------------------------------------------------------------------------------------------------------------------
def test_distance_dispatches_on_numpy(scenes):
    from wave_tracer_amd.render import distance
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    classes, mask = plan("checker_mask", height, width)
    same_result(distance(sc, classes, mask=mask, nearest=True, invert=True), sc.film_distance_host(classes, mask=mask, nearest=True, invert=True), "distance")
    got = distance(sc, mask=mask)
    assert got["n_sites"] == int((mask > 0).sum()) and got["nearest"] is None


@pytest.mark.parametrize("radius", [1, 1.5, 3])
def test_morphology_equals_scipy(scenes, radius):
    """dilate / erode / opening / closing against scipy.ndimage with the disc x² + y² <= r² as structuring element; for erosion border_value=1: the
    film's outside holds no site, so a region touching the border is not eroded from that side."""
    ndimage = pytest.importorskip("scipy.ndimage")
    from wave_tracer_amd.render import closing, dilate, erode, opening
    r = int(np.floor(radius))
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = xx ** 2 + yy ** 2 <= radius ** 2
    for width, height in SHAPES[:2]:
        sc = scenes[(width, height)]
        for name in ("perc05", "perc001", "checker_mask", "row_first", "corners_centre", "all", "none"):
            plane = sites_of(*plan(name, height, width), False, height, width)
            d, e = dilate(sc, plane, radius), erode(sc, plane, radius)
            assert d.dtype == np.bool_ and e.dtype == np.bool_
            want_d = ndimage.binary_dilation(plane, structure=disc)
            want_e = ndimage.binary_erosion(plane, structure=disc, border_value=1)
            assert np.array_equal(d, want_d) and np.array_equal(e, want_e), (name, radius)
            assert np.array_equal(opening(sc, plane, radius), ndimage.binary_dilation(want_e, structure=disc)), (name, radius)
            assert np.array_equal(closing(sc, plane, radius), ndimage.binary_erosion(want_d, structure=disc, border_value=1)), (name, radius)


def test_morphology_without_scipy(scenes):
    """what needs no scipy: radius 0 changes nothing, a pin-hole closes, a one-pixel bridge opens, the border does not erode"""
    from wave_tracer_amd.render import closing, dilate, erode, opening
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    plane = np.zeros((height, width), bool)
    plane[4:12, 3:11] = plane[4:12, 20:28] = True
    plane[8, 11:20] = True       # the bridge
    plane[7, 6] = False          # the pin-hole
    for f in (dilate, erode, opening, closing):
        assert np.array_equal(f(sc, plane, 0), plane)
    closed, opened = closing(sc, plane, 1), opening(sc, plane, 1)
    # (the cross of radius 1 also fills the four concave corners where the bridge meets the squares: every cross that holds one of them hits the plane)
    assert closed[7, 6] and closed[7, 11] and closed[9, 11] and closed[7, 19] and closed[9, 19] and closed[plane].all() and closed.sum() == plane.sum() + 5
    # (the bridge's two end pixels stay: each lies in a cross centred on the square's edge beside it)
    assert not opened[8, 12:19].any() and opened[8, 11] and opened[8, 19] and opened[5:11, 21:27].all() and not opened[~plane].any()
    assert erode(sc, np.ones((height, width), bool), 5).all() and not dilate(sc, plane & False, 5).any()


def test_nearest_segment_feeds_the_zonal_statistics(scenes):
    """The Voronoi partition of a segments plane goes to film_zonal_host as zones as it is: every pixel is in a zone, a segment's pixels are in
    their own, and the zones' n add up to the film."""
    from wave_tracer_amd.render import nearest_segment, segments, zonal
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    films = stats_films(height, width, 1, 1, 31, restate_edges("dB", -50, 10, 4))
    classes, _ = plan("perc001", height, width)
    seg = segments(sc, classes)
    assert 1 < seg["n_segments"] < 40
    zones = nearest_segment(sc, seg["segments"])
    assert zones.dtype == np.uint32 and zones.shape == (height, width) and (zones < seg["n_segments"]).all()
    assert np.array_equal(zones[seg["segments"] != NONE], seg["segments"][seg["segments"] != NONE])
    near = sc.film_distance_host(seg["segments"], nearest=True)["nearest"]
    assert np.array_equal(zones, seg["segments"].reshape(-1)[near])
    z = zonal(sc, films, SPE, zones, seg["n_segments"])
    assert int(z["n"][:, 0].sum()) == width * height and z["n_outside"] == 0 and (z["n"][:, 0] >= seg["area"]).all()
    assert np.array_equal(z["n"][:, 0], np.bincount(zones.reshape(-1), minlength=seg["n_segments"]))
    # a plane without a segment
    assert (nearest_segment(sc, np.full((height, width), NONE, np.uint32)) == NONE).all()


def test_zones_from_distance_equals_an_integer_restatement(scenes):
    from fractions import Fraction
    from wave_tracer_amd.render import zones_from_distance
    width, height = SHAPES[1]
    sc = scenes[(width, height)]
    dist2 = sc.film_distance_host(plan("corners_centre", height, width)[0])["dist2"]
    for edges in ([0, 1, 2.5, 10], [0.5, np.sqrt(2.0), 3, 20.25, 1000], [0.1, 0.2, 2], [5, 6]):
        got = zones_from_distance(dist2, edges)
        want = np.full(dist2.shape, NONE, np.uint32)
        for i in range(len(edges) - 1):
            lo, hi = Fraction(float(edges[i])) ** 2, Fraction(float(edges[i + 1])) ** 2
            inside = np.array([lo <= int(d) < hi for d in dist2.reshape(-1)]).reshape(dist2.shape)
            want[inside] = i
        assert got.dtype == np.uint32 and np.array_equal(got, want), edges
    none = sc.film_distance_host(plan("none", height, width)[0])["dist2"]
    assert (zones_from_distance(none, [0, 1e6]) == NONE).all()
    assert np.array_equal(zones_from_distance(dist2.view(np.int32), [0, 3]), zones_from_distance(dist2, [0, 3]))


# ---- the shared definitions under sanitizers ------------------------------------------------------------------------------------------------------
def test_the_header_under_the_sanitizers(tmp_path):
    """tests/film_distance_main.cpp, a stand-alone program over the header's host functions, compiled with -fsanitize=undefined,address and run as a
    child process (nothing is preloaded)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "film_distance_main"
    # the sanitizer runtimes are linked statically, so the child needs no runtime library at load time
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "wave_tracer_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "film_distance_main.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout[-2000:], run.stderr[-2000:])
