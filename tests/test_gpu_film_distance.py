"""The distance transform of a label plane on the MI355X (wtgpu_film_distance_device; csrc/kernels_distance.hip) against the host twin, bit for bit:
dist2, nearest and every field of the info.  Squared distances are integers and ties go to the smaller pixel index, so there is nothing to
tolerate.  The host twin itself is held to a brute force and to scipy by tests/test_film_distance.py, whose shapes and plans are used here — the
smallest at which something can break: 37 x 23 (one block, a partial wavefront), 130 x 67 (a row crosses a 64-lane seam, the rows end inside a
load of the column walk), 256 x 192 and 257 x 256 (a row wider than a block), 4096 x 1 (a search radius of thousands of columns, past the LDS
window, with one site at an end) and 1 x 4096 (the long column walk, no horizontal search) — every plan at every shape, with and without INVERT,
under both values of WTGPU_FILM_DISTANCE_GROUPS, and with the knob unset at 256 x 192.  Both forms give the same bits, so the form each call took
is read through wtgpu_test_film_distance_form: a silent fall-back would show nowhere else.  Nothing here provokes a fault or a loop bound."""
import numpy as np
import pytest

from test_film_distance import NONE, PLANS, plan, same_result
from test_film_segments import SHAPES, segments_scene
from test_film_stats import same_bits
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu


FORMS = {0: "plain", 1: "groups"}
DEFAULT_FORM = "groups"     # WTGPU_FILM_DISTANCE_GROUPS unset (docs/FEATURES.md has the measurement)


def _upload(sc, env):
    """the scene uploaded with its knobs read under env (the knobs are read once, at the upload)"""
    import os
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return sc.upload(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    """{(groups, W, H)}: both forms at every shape; {("default", W, H)}: the knob unset at 256 x 192"""
    d = tmp_path_factory.mktemp("gpu_film_distance")
    out = {(groups, w, h): _upload(segments_scene(d, w, h), {"WTGPU_FILM_DISTANCE_GROUPS": str(groups)}) for groups in FORMS for w, h in SHAPES}
    import os
    assert "WTGPU_FILM_DISTANCE_GROUPS" not in os.environ
    out[("default",) + SHAPES[2]] = segments_scene(d, *SHAPES[2]).upload(0)
    return out


def _d_plane(sc, a):
    """a plan's plane (read-only, shared) as a tensor on the scene's device; uint32 goes as the int32 that holds its bits"""
    return None if a is None else _to_device(sc, (np.array(a.view(np.int32) if a.dtype == np.uint32 else a),))[0]


def _host(got):
    """a device result with its planes downloaded"""
    return dict(got, dist2=got["dist2"].cpu().numpy(), nearest=None if got["nearest"] is None else got["nearest"].cpu().numpy())


def _same(sc, classes, mask, label, form, **kw):
    """device = host twin on every field, and the call took the form it must"""
    import torch
    from wave_tracer_amd.api import film_distance_form
    got = sc.film_distance_device(_d_plane(sc, classes), mask=_d_plane(sc, mask), **kw)
    assert film_distance_form(sc) == form, (label, kw, film_distance_form(sc))
    assert got["dist2"].dtype == torch.int32 and got["dist2"].is_cuda and tuple(got["dist2"].shape) == (sc.height, sc.width)
    want = sc.film_distance_host(classes, mask=mask, threads=16, **kw)
    got = _host(got)
    same_result(got, want, (label, kw))
    return got


@pytest.mark.parametrize("name", PLANS)
@pytest.mark.parametrize("width,height", SHAPES)
@pytest.mark.parametrize("groups", sorted(FORMS))
def test_device_equals_host_twin(scenes, groups, width, height, name):
    sc = scenes[(groups, width, height)]
    classes, mask = plan(name, height, width)
    for invert in (False, True):
        got = _same(sc, classes, mask, (groups, width, height, name), FORMS[groups], invert=invert, nearest=True)
        assert got["nearest"].dtype == np.int32
    if name == "none":
        assert (got["n_sites"], got["max_dist2"], got["argmax"]) == (width * height, 0, 0)       # (inverted: every pixel a site)


def test_both_forms_and_the_default_give_the_same_bits(scenes):
    """The three scenes at 256 x 192 directly against each other, and the form the knob's default takes."""
    width, height = SHAPES[2]
    for name in PLANS:
        classes, mask = plan(name, height, width)
        for invert in (False, True):
            a = _same(scenes[(0, width, height)], classes, mask, name, "plain", invert=invert, nearest=True)
            b = _same(scenes[(1, width, height)], classes, mask, name, "groups", invert=invert, nearest=True)
            c = _same(scenes[("default", width, height)], classes, mask, name, DEFAULT_FORM, invert=invert, nearest=True)
            same_result(b, a, name)
            same_result(c, a, name)


def test_without_nearest_nothing_else_is_written(scenes):
    """nearest=False gives the same dist2 and info and makes no second plane; at the C interface a NULL d_nearest leaves a plane of the caller's alone"""
    import ctypes as C
    import torch
    from wave_tracer_amd.api import FilmDistanceInfo, FilmDistanceSpec, load_library
    width, height = SHAPES[1]
    for groups in FORMS:
        sc = scenes[(groups, width, height)]
        for name in ("perc001", "checker_mask"):
            classes, mask = plan(name, height, width)
            a = _same(sc, classes, mask, name, FORMS[groups], nearest=True)
            b = _same(sc, classes, mask, name, FORMS[groups], nearest=False)
            assert b["nearest"] is None
            same_result(b, dict(a, nearest=None), name)
        # guard words around dist2: the kernels write the plane and nothing beside it
        n = width * height
        buf = torch.full((n + 512,), 77, dtype=torch.int32, device=torch.device("cuda", 0))
        info = FilmDistanceInfo()
        rc = load_library().wtgpu_film_distance_device(sc.handle, None, C.byref(FilmDistanceSpec(0)), _d_plane(sc, classes).data_ptr(), None, buf[256:256 + n].data_ptr(), None, C.byref(info))
        torch.cuda.synchronize()
        assert rc == 0 and (buf[:256] == 77).all().item() and (buf[256 + n:] == 77).all().item()
        assert same_bits(buf[256:256 + n].cpu().numpy().reshape(height, width), sc.film_distance_host(classes)["dist2"].view(np.int32))


def test_repeated_calls_and_a_small_film_after_a_large_one(built, tmp_path):
    """The scratch is sized by the call and grown when a later call needs more: the same plan twice on one scene gives the same; a scene's calls do
    not disturb another's."""
    big = segments_scene(tmp_path, *SHAPES[3]).upload(0)
    small = segments_scene(tmp_path, *SHAPES[0]).upload(0)
    for _ in range(2):
        for sc in (big, small):
            for name in ("perc001", "perc05", "corners_centre"):
                classes, mask = plan(name, sc.height, sc.width)
                a = _same(sc, classes, mask, name, DEFAULT_FORM, nearest=True)
                b = _same(sc, classes, mask, name, DEFAULT_FORM, nearest=True, invert=True)
                c = _same(sc, classes, mask, name, DEFAULT_FORM, nearest=True)
                same_result(c, a, name)
                assert a["n_sites"] + b["n_sites"] == sc.width * sc.height


def test_shadows_and_holes_of_a_rendered_film(built):
    """The bundled etoile at res 64: line_of_sight's n_visible == 0 plane as classes — the distance to the nearest shadow, and the depth inside it;
    nearest_segment of coverage_holes' segments fed to film_zonal_device, equal to the host twins on the downloaded film."""
    import torch
    from wave_tracer_amd import Scene, imageio
    from wave_tracer_amd.render import alloc_films, coverage_holes, distance, nearest_segment, zonal
    dev = torch.device("cuda", 0)
    sc = Scene("etoile", res=64, mesh_detail=0).upload(0)
    d_visible = sc.line_of_sight(0, 1, maps=(), ids=("n_visible",))["n_visible"].contiguous()
    d_classes = torch.where(d_visible == 0, 1, -1).to(torch.int32).contiguous()
    classes = d_classes.cpu().numpy().view(np.uint32)
    assert 0 < int((classes == 1).sum()) < classes.size
    for invert in (False, True):
        got = _host(distance(sc, d_classes, nearest=True, invert=invert))
        want = distance(sc, classes, nearest=True, invert=invert)
        same_result(got, want, ("shadows", invert))
        assert got["n_sites"] == int(((classes == 1) != invert).sum()) and 0 < got["max_dist2"] < NONE
    d_films = alloc_films(sc, dev)
    sc.render_into(*d_films, 0, 4, 21, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    films = tuple(t.cpu().numpy() for t in d_films)
    stats = sc.film_stats_device(*d_films, 4, scale="dB", range=None, bins=256)
    median = float(np.ravel(imageio.percentiles(stats, 50))[0])
    holes_d, holes_h = coverage_holes(sc, d_films, 4, median, min_area=3), coverage_holes(sc, films, 4, median, min_area=3)
    K = holes_d["n_segments"]
    assert K == holes_h["n_segments"] >= 1
    zones_d, zones_h = nearest_segment(sc, holes_d["segments"]), nearest_segment(sc, holes_h["segments"])
    assert zones_d.dtype == torch.int32 and zones_d.is_cuda and same_bits(zones_d.cpu().numpy().view(np.uint32), zones_h)
    assert (zones_h < K).all()
    z_d, z_h = zonal(sc, d_films, 4, zones_d, K), zonal(sc, films, 4, zones_h, K)
    for k in ("n", "min", "max", "sum"):
        assert same_bits(z_d[k], z_h[k]), k
    assert int(z_d["n"][:, 0].sum()) == sc.width * sc.height and z_d["n_outside"] == 0


def test_the_helpers_on_the_device(scenes):
    """dilate / erode / opening / closing and zones_from_distance on torch planes equal the same on numpy planes"""
    import torch
    from wave_tracer_amd.render import closing, dilate, distance, erode, opening, zones_from_distance
    width, height = SHAPES[1]
    sc = scenes[(1, width, height)]
    classes, _ = plan("perc05", height, width)
    plane = classes != NONE
    d_plane = torch.from_numpy(plane).to(torch.device("cuda", 0))
    for f in (dilate, erode, opening, closing):
        for radius in (1, 1.5, 3):
            got = f(sc, d_plane, radius)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), f(sc, plane, radius)), (f.__name__, radius)
    sparse = plan("corners_centre", height, width)[0]
    d2_d, d2_h = distance(sc, _d_plane(sc, sparse))["dist2"], distance(sc, sparse)["dist2"]
    for edges in ([0, 1, 2.5, 10], [0.5, 3, 20.25, 1000]):
        assert same_bits(zones_from_distance(d2_d, edges).cpu().numpy().view(np.uint32), zones_from_distance(d2_h, edges))
    none = distance(sc, _d_plane(sc, plan("none", height, width)[0]))["dist2"]
    assert (zones_from_distance(none, [0, 1e6]) == -1).all().item()


def test_distance_between_renders_changes_nothing(built):
    """As test_gpu_film_segments.py's: the call counts nothing and leaves the films alone."""
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import cell_zones
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_films = _to_device(sc, a)
    zones, Z = cell_zones(sc.height, sc.width, 8)
    classes = np.where(zones % 3 == 0, zones, NONE).astype(np.uint32)
    got = sc.film_distance_device(_d_plane(sc, classes), nearest=True)
    assert all(v == 0 for v in sc.counters().values()) and got["n_sites"] == int((classes != NONE).sum()) > 0
    same_result(_host(got), sc.film_distance_host(classes, nearest=True), "between renders")
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_films))


def test_refusals_on_the_device_side(scenes, tmp_path):
    """A scene that is not uploaded: WTGPU_ERR_INVALID (1) from the entry point itself, with the message, and the Python method says the same before
    it gets there; planes of another dtype, shape, device or layout are refused in Python."""
    import ctypes as C
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmDistanceInfo, FilmDistanceSpec, film_distance_form, load_library
    width, height = SHAPES[0]
    sc = segments_scene(tmp_path, width, height)
    dev = torch.device("cuda", 0)
    z = torch.zeros((height, width), dtype=torch.int32, device=dev)
    out = torch.full((height, width), 5, dtype=torch.int32, device=dev)
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_distance_device(z)
    assert film_distance_form(sc) is None      # no call has launched anything
    lib = load_library()
    info = FilmDistanceInfo()
    rc = lib.wtgpu_film_distance_device(sc.handle, None, C.byref(FilmDistanceSpec(0)), z.data_ptr(), None, out.data_ptr(), None, C.byref(info))
    assert rc == 1 and lib.wtgpu_last_error() == b"film_distance: scene not uploaded" and (out == 5).all().item()
    up = scenes[(1, width, height)]
    for bad in (z.long(), z.float(), z[:, :-1], z.cpu(), z.t().contiguous().t()):
        with pytest.raises(ValueError, match="classes: a contiguous torch.int32"):
            up.film_distance_device(bad)
    m = torch.ones((height, width), dtype=torch.float32, device=dev)
    for bad in (m.double(), m[:-1], m.cpu()):
        with pytest.raises(ValueError, match="mask: a contiguous torch.float32"):
            up.film_distance_device(z, mask=bad)
    got = up.film_distance_device(None, mask=m)
    assert (got["n_sites"], got["max_dist2"], got["argmax"]) == (width * height, 0, 0) and got["nearest"] is None
