"""Connected segments of a label plane (wt/film_segments.h: wtgpu_film_segments_host; render.segments, coverage_holes) on the CPU: the host twin
against a flood fill written here (a breadth-first search from every unvisited member in row-major order, which yields the canonical numbering
directly; it calls nothing of the library) and, where scipy imports, against scipy.ndimage.label per class.  tests/test_gpu_film_segments.py runs
the device kernels against the host twin on the same shapes and plans.

There is no tolerance anywhere: a segment is a set of pixels and its number is fixed by its smallest pixel index, so the plane, the four counts
and every field of every record are integers that must be equal."""
import functools
import os
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest

from test_film_stats import F32, SPE, stats_films, stats_scene, restate_edges
from test_sensor_mask import _write
from test_tonemap import MONO, film_xml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
# (W, H): one block with a partial last wavefront and rows that are no multiples of 64; runs that cross a 64-lane seam and a row end inside one
# load; 48 blocks; 257 chunks, so the scan of the chunk counts takes a second turn; one row; one column
SHAPES = [(37, 23), (130, 67), (256, 192), (257, 256), (4096, 1), (1, 4096)]
PLANS = ("one", "one7", "checker_holes", "checker_two", "spiral", "snake", "comb", "rings", "perc1", "perc2", "perc3", "random5", "checker_mask", "mask_none")
INFO = ("n_segments", "n_dropped", "n_members", "n_dropped_pixels")
RECORD = ("klass", "area", "first", "bbox", "centroid")


def cases():
    """every plan at every shape"""
    return [(w, h, plan) for w, h in SHAPES for plan in PLANS]


# ---- plans ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan(name, height, width):
    rng = np.random.default_rng(len(name) * 1000 + height + width)
    yy, xx = np.mgrid[0:height, 0:width]
    classes, mask = None, None
    if name == "one7":
        classes = np.full((height, width), 7, np.uint32)
    elif name == "checker_holes":       # one colour is no member: every member stands alone, all of them join by their corners
        classes = np.where((yy + xx) % 2 == 0, 3, NONE)
    elif name == "checker_two":         # two colours, two classes: a segment per pixel, one per colour by the corners
        classes = (yy + xx) % 2
    elif name == "spiral":              # a one-pixel path that winds inwards, and the one-pixel gap beside it
        classes = np.zeros((height, width), np.uint32)
        y = x = 0
        dy, dx = 0, 1
        classes[0, 0] = 1
        free = lambda v, u: not (0 <= v < height and 0 <= u < width) or classes[v, u] == 0
        while True:
            for _ in range(2):
                if 0 <= y + dy < height and 0 <= x + dx < width and classes[y + dy, x + dx] == 0 and free(y + 2 * dy, x + 2 * dx):
                    y, x = y + dy, x + dx
                    classes[y, x] = 1
                    break
                dy, dx = dx, -dy
            else:
                break
    elif name == "snake":               # every other row, joined at alternating ends: one segment with the longest chains of parents
        classes = np.where(yy % 2 == 0, 1, NONE)
        odd = np.arange(1, height, 2)
        classes[odd, np.where(odd % 4 == 1, width - 1, 0)] = 1
    elif name == "comb":                # teeth that join in the last row only: the merges are found late
        classes = np.where((xx % 2 == 0) | (yy == height - 1), 2, NONE)
    elif name == "rings":
        classes = np.maximum(abs(yy - height // 2), abs(xx - width // 2)) % 3
    elif name.startswith("perc"):       # site percolation at the critical density of the square lattice
        classes = np.where(np.random.default_rng(int(name[4:])).random((height, width)) < 0.593, 1, NONE)
    elif name in ("random5", "checker_mask", "mask_none"):
        classes = np.where(rng.random((height, width)) < 0.1, NONE, rng.integers(0, 5, (height, width)))
    elif name != "one":
        raise KeyError(name)
    if name == "checker_mask":          # excluded: zeros, negatives, -0 and a NaN
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


# ---- the flood fill ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flood(name, height, width, diagonal):
    classes, mask = plan(name, height, width)
    cls = (np.zeros((height, width), np.uint32) if classes is None else classes).astype(np.int64)
    if mask is not None:
        cls = np.where(mask > 0, cls, NONE)         # (a NaN is not > 0)
    cls = cls.reshape(-1).tolist()
    n = height * width
    label = [-1] * n
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if diagonal else [])
    segs = []
    for p0 in range(n):
        c = cls[p0]
        if c == NONE or label[p0] >= 0:
            continue
        k = len(segs)
        label[p0] = k
        queue = deque([p0])
        area = sx = sy = 0
        x0 = y0 = n
        x1 = y1 = -1
        while queue:
            p = queue.popleft()
            y, x = divmod(p, width)
            area, sx, sy = area + 1, sx + x, sy + y
            x0, y0, x1, y1 = min(x0, x), min(y0, y), max(x1, x), max(y1, y)
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if 0 <= v < height and 0 <= u < width:
                    q = v * width + u
                    if label[q] < 0 and cls[q] == c:
                        label[q] = k
                        queue.append(q)
        segs.append((c, area, p0, x0, y0, x1, y1, sx, sy))
    return np.array(label, np.int64), segs, sum(1 for c in cls if c != NONE)


def flood(name, height, width, diagonal=False, min_area=1, max_records=65536):
    """What the library must return for a plan, from the flood fill at min_area = 1: the dropped segments leave and the rest move up."""
    label, segs, n_members = _flood(name, height, width, bool(diagonal))
    keep = [s[1] >= max(min_area, 1) for s in segs]
    new = np.cumsum(keep) - 1
    lut = np.append(np.where(keep, new, NONE), NONE).astype(np.uint32)     # (label -1: no member)
    kept = [s for s, k in zip(segs, keep) if k][:min(max_records, height * width)]
    col = lambda i, dt: np.array([s[i] for s in kept], dt)
    area = col(1, np.float64)
    return {"segments": lut[label].reshape(height, width), "n_segments": int(sum(keep)), "n_dropped": len(segs) - int(sum(keep)), "n_members": n_members,
            "n_dropped_pixels": sum(s[1] for s, k in zip(segs, keep) if not k), "klass": col(0, np.uint32), "area": col(1, np.uint32), "first": col(2, np.uint32),
            "bbox": np.array([s[3:7] for s in kept], np.uint32).reshape(-1, 4), "centroid": np.stack([col(7, np.float64) / area, col(8, np.float64) / area], axis=1)}


def same_result(got, want, label, plane=None):
    """every count, every record field and the plane (got's, or `plane`, as uint32 bits) are equal"""
    for k in INFO:
        assert got[k] == want[k], (label, k, got[k], want[k])
    for k in RECORD:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (label, k, got[k][:4], want[k][:4])
    seg = np.asarray(got["segments"] if plane is None else plane).view(np.uint32)
    assert seg.shape == want["segments"].shape and np.array_equal(seg, want["segments"].view(np.uint32)), (label, "segments", np.argwhere(seg != want["segments"])[:4].tolist())


def options(name):
    """(min_area, max_records) beside the plain call: a plan's share of min_area 2 / 50 and max_records 0 / 3"""
    return [(1, 65536)] + {"perc1": [(2, 3), (50, 0)], "perc2": [(50, 3)], "random5": [(2, 0), (50, 65536)], "checker_two": [(2, 3)], "spiral": [(50, 3)],
                           "checker_mask": [(2, 3)]}.get(name, [])


def segments_scene(d, width, height):
    """A scene whose sensor has the shape: tests/test_film_stats.py's, with a virtual-plane sensor where the film is one pixel wide or high (a
    perspective camera of such a film has no projection)."""
    if min(width, height) > 1:
        return stats_scene(d, 1, width, height)
    from wave_tracer_amd import Scene
    camera = '<sensor type="perspective"><quantity name="fov" value="60°"/>'
    text = film_xml(response=MONO, width=width, height=height)
    assert text.count(camera) == 1
    sc = Scene.from_xml(_write(d, f"plane{width}x{height}.xml", text.replace(camera, '<sensor type="virtual_plane"><quantity name="alpha" value=".001°"/><quantity name="extent" value="4 m, 4 m"/>')))
    assert (sc.width, sc.height, sc.spectral_channels, sc.stokes) == (width, height, 1, 1)
    return sc


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_segments")
    return {(w, h): segments_scene(d, w, h) for w, h in SHAPES}


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,name", cases())
def test_host_twin_equals_the_flood_fill(scenes, width, height, name):
    sc = scenes[(width, height)]
    classes, mask = plan(name, height, width)
    for diagonal in (False, True):
        for min_area, max_records in options(name):
            got = sc.film_segments_host(classes, mask=mask, diagonal=diagonal, min_area=min_area, max_records=max_records, threads=1)
            want = flood(name, height, width, diagonal, min_area, max_records)
            same_result(got, want, (name, diagonal, min_area, max_records))
            assert got["segments"].dtype == np.uint32 and len(got["area"]) == min(got["n_segments"], max_records)
            assert got["n_members"] == got["n_dropped_pixels"] + int((got["segments"] != NONE).sum())


def test_what_the_plans_are_known_to_give(scenes):
    """The counts that need no flood fill: one segment for one class; a checkerboard of members stands alone pixel by pixel and joins by the corners;
    the snake and the comb are one segment each; an all-excluding mask leaves nothing."""
    for width, height in SHAPES[:2]:
        sc = scenes[(width, height)]
        n = width * height
        k = lambda name, **kw: sc.film_segments_host(*plan(name, height, width)[:1], mask=plan(name, height, width)[1], **kw)
        for name in ("one", "one7"):
            got = k(name)
            assert (got["n_segments"], got["n_members"], got["area"].tolist(), got["bbox"].tolist()) == (1, n, [n], [[0, 0, width - 1, height - 1]])
            assert got["centroid"].tolist() == [[(width - 1) / 2, (height - 1) / 2]] and got["klass"][0] == (7 if name == "one7" else 0) and not got["segments"].any()
        holes = k("checker_holes")
        assert holes["n_segments"] == holes["n_members"] == (n + 1) // 2 and (holes["area"] == 1).all() and k("checker_holes", diagonal=True)["n_segments"] == 1
        assert k("checker_two")["n_segments"] == n and k("checker_two", diagonal=True)["n_segments"] == 2
        assert k("checker_two", min_area=2)["n_segments"] == 0 and k("checker_two", min_area=2)["n_dropped_pixels"] == n
        for name in ("snake", "comb"):
            got = k(name)
            assert got["n_segments"] == 1 and got["area"][0] == got["n_members"] and got["bbox"].tolist() == [[0, 0, width - 1, height - 1]]
        spiral = k("spiral")
        assert spiral["n_segments"] == 2 and spiral["first"].tolist() == [0, width] and spiral["klass"].tolist() == [1, 0]
        none = k("mask_none")
        assert (none["n_segments"], none["n_members"], none["n_dropped"], len(none["area"])) == (0, 0, 0, 0) and (none["segments"] == NONE).all()
        # min_area 0 is min_area 1
        assert k("perc1", min_area=0)["n_segments"] == k("perc1")["n_segments"] > k("perc1", min_area=50)["n_segments"] > 0


@pytest.mark.parametrize("width,height", SHAPES)
def test_host_twin_equals_scipy_label(scenes, width, height):
    """scipy.ndimage.label per class with the matching structure: the same number of components, and a one-to-one map between its (class, label)
    pairs and the twin's numbers."""
    ndimage = pytest.importorskip("scipy.ndimage")
    sc = scenes[(width, height)]
    for name in PLANS:
        classes, mask = plan(name, height, width)
        cls = np.zeros((height, width), np.uint32) if classes is None else classes
        member = (cls != NONE) & (True if mask is None else mask > 0)
        for diagonal in (False, True):
            got = sc.film_segments_host(classes, mask=mask, diagonal=diagonal)
            seg = got["segments"]
            assert np.array_equal(seg != NONE, member)
            pairs, total = set(), 0
            for c in np.unique(cls[member]):
                lab, n = ndimage.label(member & (cls == c), structure=np.ones((3, 3)) if diagonal else None)
                total += n
                pairs |= set(zip(seg[lab > 0].tolist(), (lab[lab > 0].astype(np.int64) + (int(c) << 32)).tolist()))
            assert total == got["n_segments"] == len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}), (name, diagonal, total, got["n_segments"])


def test_the_result_does_not_depend_on_the_threads(scenes):
    width, height = SHAPES[1]
    sc = scenes[(width, height)]
    for name in ("perc2", "random5", "checker_mask"):
        classes, mask = plan(name, height, width)
        a = sc.film_segments_host(classes, mask=mask, diagonal=True, min_area=2, threads=1)
        b = sc.film_segments_host(classes, mask=mask, diagonal=True, min_area=2, threads=5)
        same_result(a, b, name)


def test_int32_bits_are_taken_like_uint32(scenes):
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    classes, _ = plan("random5", height, width)
    same_result(sc.film_segments_host(classes.view(np.int32)), sc.film_segments_host(classes), "int32")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_say_why(scenes):
    import ctypes as C
    from wave_tracer_amd.api import FILM_SEGMENT_FIELDS, FilmSegmentsInfo, FilmSegmentsSpec, load_library
    lib = load_library()
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    seg = np.full((height, width), 5, np.uint32)
    rec = np.zeros(4, np.dtype(FILM_SEGMENT_FIELDS))
    info = FilmSegmentsInfo(9, 9, 9, 9)

    def refused(spec, segments, info_, records, message):
        rc = lib.wtgpu_film_segments_host(sc.handle, C.byref(spec), None, None, 1, segments, info_, records)
        assert (rc, lib.wtgpu_last_error().decode()) == (1, message)
        # the device entry point refuses the same things first, before it asks for an upload
        rc = lib.wtgpu_film_segments_device(sc.handle, None, C.byref(spec), None, None, segments, info_, records)
        assert (rc, lib.wtgpu_last_error().decode()) == (1, message)
    ok = FilmSegmentsSpec(0, 1, 4, 0)
    refused(ok, None, C.byref(info), rec.ctypes.data, "film_segments: segments and info expected (one of them is NULL)")
    refused(ok, seg.ctypes.data, None, rec.ctypes.data, "film_segments: segments and info expected (one of them is NULL)")
    refused(ok, seg.ctypes.data, C.byref(info), None, "film_segments: max_records 4 without records (records is NULL)")
    for flags in (2, 3, 0x80000000):
        refused(FilmSegmentsSpec(flags, 1, 4, 0), seg.ctypes.data, C.byref(info), rec.ctypes.data, f"film_segments: flags 0 or 1 (DIAGONAL) expected, got {flags}")
    # the device call without an upload
    rc = lib.wtgpu_film_segments_device(sc.handle, None, C.byref(ok), None, None, seg.ctypes.data, C.byref(info), rec.ctypes.data)
    assert (rc, lib.wtgpu_last_error().decode()) == (1, "film_segments: scene not uploaded")
    assert (seg == 5).all() and not rec["area"].any() and info.n_segments == 9      # nothing was written
    # max_records 0 goes without records
    rc = lib.wtgpu_film_segments_host(sc.handle, C.byref(FilmSegmentsSpec(1, 1, 0, 0)), None, None, 1, seg.ctypes.data, C.byref(info), None)
    assert rc == 0 and (info.n_segments, info.n_members) == (1, width * height) and not seg.any()


def test_a_sensor_of_2_to_the_31_pixels_is_refused(built, tmp_path):
    """Pixel indices and areas are 32-bit.  A scene holds nothing per pixel and the entry point refuses before it reads a plane; 65536 x 32767 passes
    this check, and the next refusal in line answers."""
    import ctypes as C
    from wave_tracer_amd.api import FilmSegmentsInfo, FilmSegmentsSpec, load_library
    lib = load_library()
    dummy, info = np.zeros(16, np.uint32), FilmSegmentsInfo()
    for height, message in ((32768, "film_segments: a sensor of 2^31 pixels or more (pixel indices and areas are 32-bit)"),
                            (32767, "film_segments: max_records 1 without records (records is NULL)")):
        sc = stats_scene(tmp_path, 1, 65536, height)
        spec = FilmSegmentsSpec(0, 1, 0 if height == 32768 else 1, 0)
        for rc in (lib.wtgpu_film_segments_host(sc.handle, C.byref(spec), None, None, 1, dummy.ctypes.data, C.byref(info), None),
                   lib.wtgpu_film_segments_device(sc.handle, None, C.byref(spec), None, None, dummy.ctypes.data, C.byref(info), None)):
            assert rc == 1
        assert lib.wtgpu_last_error().decode() == message
    assert not dummy.any()


def test_planes_of_another_kind_are_refused_in_python(scenes):
    from wave_tracer_amd import WtgpuError
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    z = np.zeros((height, width), np.uint32)
    for bad in (z.astype(np.int64), z.astype(np.float32), z[:, :-1], z.T, np.zeros((width, height), np.uint32).T, z.tolist()):
        with pytest.raises(ValueError, match="film_segments_host: classes: a contiguous int32 or uint32 array"):
            sc.film_segments_host(bad)
    m = np.ones((height, width), F32)
    for bad in (m.astype(np.float64), m[:-1], np.ones((width, height), F32).T):
        with pytest.raises(ValueError, match="film_segments_host: mask: a contiguous float32 array"):
            sc.film_segments_host(z, mask=bad)
    with pytest.raises(ValueError, match="must not be negative"):
        sc.film_segments_host(z, min_area=-1)
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_segments_device(None)


# ---- the bound of the union-find's walk (the kernels' find, on the host) ---------------------------------------------------------------------------
def test_find_stops_at_its_bound_and_flags_it():
    """The device's loops carry a step bound so that a bug ends as a refusal, never as a hung card.  No test provokes that on the GPU; the same find
    runs here on hand-made parents: a chain of 9 below its root needs 10 loads; a parent above its child is flagged at once."""
    from wave_tracer_amd.api import film_segments_find
    chain = np.array([0, 0, 1, 2, 3, 4, 5, 6, 7, 8], np.uint32)
    for x in range(10):
        assert film_segments_find(chain, x, x + 1) == (0, False)            # x hops and the look at the root
        assert film_segments_find(chain, x, 10) == (0, False)
        if x:
            assert film_segments_find(chain, x, x) == (0, True)             # at the root, but it has not seen so
        for bound in range(x):
            assert film_segments_find(chain, x, bound) == (x - bound, True)
    forest = np.array([0, 1, 1, 0, 2, 5, 5], np.uint32)
    assert [film_segments_find(forest, x, 7)[0] for x in range(7)] == [0, 1, 1, 0, 1, 5, 5]
    cycle = np.array([0, 2, 1, 5, 3, 4], np.uint32)                         # 1 -> 2: a parent above its child; 3 -> 5 likewise
    assert film_segments_find(cycle, 1, 1000) == (1, True) and film_segments_find(cycle, 2, 1000) == (1, True)
    assert film_segments_find(cycle, 4, 1000) == (3, True) and film_segments_find(cycle, 0, 1000) == (0, False)


def test_find_refuses_parents_beyond_the_array(built):
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import film_segments_find
    with pytest.raises(WtgpuError, match=r"parent\[2\] is not below n"):
        film_segments_find(np.array([0, 0, 9], np.uint32), 1, 5)
    with pytest.raises(WtgpuError, match="x < n"):
        film_segments_find(np.array([0, 0], np.uint32), 2, 5)


# ---- the helpers --------------------------------------------------------------------------------------------------------------------------------
def test_segments_feed_the_zonal_statistics(scenes):
    """The plane goes to film_zonal_host as zones as it is: every zone's n is the segment's area, and the dropped pixels are outside."""
    from wave_tracer_amd.render import segments, zonal
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    films = stats_films(height, width, 1, 1, 31, restate_edges("dB", -50, 10, 4))
    for name, kw in (("perc1", {}), ("random5", dict(diagonal=True, min_area=3)), ("checker_mask", dict(min_area=2))):
        classes, mask = plan(name, height, width)
        got = segments(sc, classes, mask=mask, **kw)
        same_result(got, flood(name, height, width, kw.get("diagonal", False), kw.get("min_area", 1)), name)
        z = zonal(sc, films, SPE, got["segments"], got["n_segments"], mask=mask)
        included = width * height if mask is None else int((mask > 0).sum())       # (zonal's members are the mask's: a pixel of no class is outside too)
        assert np.array_equal(z["n"][:, 0], got["area"]) and z["n_outside"] == included - int(got["area"].sum()) >= got["n_dropped_pixels"]
    # without classes the mask alone says what a member is
    _, mask = plan("checker_mask", height, width)
    got = segments(sc, mask=mask)
    assert got["n_members"] == int((mask > 0).sum()) and (got["klass"] == 0).all() and np.array_equal(got["segments"] != NONE, mask > 0)


def test_coverage_holes_on_numpy_films(scenes):
    """The holes of a film whose developed values are known: the class plane restated here, the segments against the flood fill's twin, and a hole's
    zonal n equal to its record's area."""
    from wave_tracer_amd.render import coverage_holes, develop
    width, height = SHAPES[0]
    sc = scenes[(width, height)]
    films = stats_films(height, width, 1, 1, 32, restate_edges("dB", -50, 10, 4), infinities=True)
    x = develop(sc, *films, SPE).reshape(height, width)
    assert np.isnan(x).any() and (x < 0.1).any() and (x >= 0.1).any()
    for scale, threshold, thr in (("dB", -10.0, F32(10.0 ** -1.0)), ("linear", 0.1, F32(0.1))):
        for below in (True, False):
            kw = dict(min_area=2, diagonal=True) if below else {}
            got = coverage_holes(sc, films, SPE, threshold, scale=scale, below=below, **kw)
            assert got["threshold"] == thr
            inside = (x < thr) if below else (x >= thr)
            classes = np.where(inside, 1, NONE).astype(np.uint32)
            want = sc.film_segments_host(classes, **kw)
            same_result(got, want, (scale, below))
            assert got["n_segments"] > (0 if below else 1) and got["n_members"] == int(inside.sum()) and (got["klass"] == 1).all()
            assert np.array_equal(got["zonal"]["n"][:, 0], got["area"]) and got["zonal"]["n_outside"] == width * height - int(got["area"].sum())
            # every element of a hole lies on the hole's side of the threshold
            side = got["zonal"]["max"][:, 0] < thr if below else got["zonal"]["min"][:, 0] >= thr
            assert side.all()
    # a developed film is taken as it is; where every hole is dropped the zonal part says so
    dev = np.ascontiguousarray(x.reshape(height, width, 1, 1))
    a, b = coverage_holes(sc, dev, None, 0.1, scale="linear"), coverage_holes(sc, films, SPE, 0.1, scale="linear")
    same_result(a, b, "developed")
    empty = coverage_holes(sc, films, SPE, 0.1, scale="linear", min_area=width * height)
    assert empty["n_segments"] == 0 and empty["zonal"] is None and empty["zonal_skipped"] == "no segments"
    with pytest.raises(ValueError, match="scale 'dB' or 'linear'"):
        coverage_holes(sc, films, SPE, 0.1, scale="log")
    with pytest.raises(ValueError, match="channel 1 / stokes_component 0 out of range"):
        coverage_holes(sc, films, SPE, 0.1, channel=1)


# ---- the shared definitions under sanitizers ------------------------------------------------------------------------------------------------------
def test_the_header_under_the_sanitizers(tmp_path):
    """tests/film_segments_main.cpp, a stand-alone program over the header's host functions, compiled with -fsanitize=undefined,address and run as a
    child process (nothing is preloaded)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "film_segments_main"
    # the sanitizer runtimes are linked statically, so the child needs no runtime library at load time
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "wave_tracer_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "film_segments_main.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout[-2000:], run.stderr[-2000:])
