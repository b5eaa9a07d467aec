"""Connected segments of a label plane on the MI355X (wtgpu_film_segments_device; csrc/kernels_segments.hip) against the host twin, bit for bit: the
plane, the four counts and every field of every record.  The answer is canonical — a segment is a set of pixels, numbered by its smallest pixel
index — so there is nothing to tolerate, whatever order the union-find's atomics land in.  The host twin itself is held to a flood fill and to
scipy.ndimage.label by tests/test_film_segments.py, whose shapes and plans are used here: 37 x 23 (one block, a partial last wavefront), 130 x 67
(runs that cross a 64-lane seam, row ends inside a load), 256 x 192 (48 blocks), 257 x 256 (257 chunks: the scan of the chunk counts takes a second
turn), one row and one column of 4096 — every plan at every shape (the host twin needs no flood fill), in both forms of the first two phases:
WTGPU_FILM_SEGMENTS_TILED=1 (a block labels a 64 x 32 tile in LDS, the global merge unions across tile borders) and 0 (row runs of 64 pixels, every
other link in global memory).  Both forms give the same bits, so the form each call took is read through wtgpu_test_film_segments_form: a silent
fall-back would show nowhere else.  Every call's overflow word — set where a union-find loop hits its step bound — is read through the test
hook and must be zero; nothing here provokes it (its logic is tested on the CPU)."""
import numpy as np
import pytest

from test_film_segments import NONE, PLANS, SHAPES, options, plan, same_result, segments_scene
from test_film_stats import same_bits
from test_film_stats import to_device as _to_device

pytestmark = pytest.mark.gpu


FORMS = {0: "global", 1: "tiled"}


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
    """{(tiled, W, H)}: both forms at every shape; {("default", W, H)}: the knob unset at 256 x 192"""
    d = tmp_path_factory.mktemp("gpu_film_segments")
    out = {(tiled, w, h): _upload(segments_scene(d, w, h), {"WTGPU_FILM_SEGMENTS_TILED": str(tiled)}) for tiled in FORMS for w, h in SHAPES}
    import os
    assert "WTGPU_FILM_SEGMENTS_TILED" not in os.environ
    out[("default",) + SHAPES[2]] = segments_scene(d, *SHAPES[2]).upload(0)
    return out


def _d_plane(sc, a):
    """a plan's plane (read-only, shared) as a tensor on the scene's device; uint32 goes as the int32 that holds its bits"""
    return None if a is None else _to_device(sc, (np.array(a.view(np.int32) if a.dtype == np.uint32 else a),))[0]


def _same(sc, classes, mask, label, form, **kw):
    """device = host twin on every field, the call took the form it must and no loop hit its bound"""
    from wave_tracer_amd.api import film_segments_form
    got = sc.film_segments_device(_d_plane(sc, classes), mask=_d_plane(sc, mask), **kw)
    assert film_segments_form(sc) == (form, 0), (label, kw, film_segments_form(sc))
    want = sc.film_segments_host(classes, mask=mask, threads=16, **kw)
    import torch
    assert got["segments"].dtype == torch.int32 and got["segments"].is_cuda
    same_result(got, want, (label, kw), plane=got["segments"].cpu().numpy())
    return got


@pytest.mark.parametrize("name", PLANS)
@pytest.mark.parametrize("width,height", SHAPES)
@pytest.mark.parametrize("tiled", sorted(FORMS))
def test_device_equals_host_twin(scenes, tiled, width, height, name):
    sc = scenes[(tiled, width, height)]
    classes, mask = plan(name, height, width)
    for diagonal in (False, True):
        for min_area, max_records in options(name):
            got = _same(sc, classes, mask, (tiled, width, height, name), FORMS[tiled], diagonal=diagonal, min_area=min_area, max_records=max_records)
            assert len(got["area"]) == min(got["n_segments"], max_records)
    if name == "snake":
        assert got["n_segments"] == 1 and got["area"][0] == got["n_members"]


def test_both_forms_and_the_default_give_the_same_bits(scenes):
    """The three scenes at 256 x 192 directly against each other; the knob's default is the global form (measured level or faster)."""
    width, height = SHAPES[2]
    for name in ("perc2", "spiral", "rings", "checker_mask"):
        classes, mask = plan(name, height, width)
        a = _same(scenes[(0, width, height)], classes, mask, name, "global", diagonal=True, min_area=2)
        b = _same(scenes[(1, width, height)], classes, mask, name, "tiled", diagonal=True, min_area=2)
        c = _same(scenes[("default", width, height)], classes, mask, name, "global", diagonal=True, min_area=2)
        for other in (b, c):
            same_result(other, dict(a, segments=a["segments"].cpu().numpy().view(np.uint32)), name, plane=other["segments"].cpu().numpy())


def test_a_call_after_a_larger_one_and_repeated_calls(scenes):
    """The scratch grows with the calls and is cleared by each: the same plan twice, and a small max_records after a large one, give the same."""
    width, height = SHAPES[2]
    sc = scenes[(1, width, height)]
    classes, mask = plan("perc1", height, width)
    a = _same(sc, classes, mask, "first", "tiled", max_records=width * height)
    b = _same(sc, classes, mask, "second", "tiled", max_records=5)
    c = _same(sc, classes, mask, "third", "tiled", max_records=width * height)
    assert a["n_segments"] == b["n_segments"] == c["n_segments"] > 5 and len(b["area"]) == 5 and np.array_equal(a["area"], c["area"])
    assert same_bits(a["segments"].cpu().numpy(), b["segments"].cpu().numpy())


def test_coverage_holes_of_a_rendered_film(built):
    """The bundled etoile at res 64: the holes below the film's median (film_stats_device's histogram) on the device against the twins on the
    downloaded film; line_of_sight's n_visible == 0 plane as classes — one segment per shadow."""
    import torch
    from wave_tracer_amd import Scene, imageio
    from wave_tracer_amd.api import film_segments_form
    from wave_tracer_amd.render import alloc_films, coverage_holes, segments
    dev = torch.device("cuda", 0)
    sc = Scene("etoile", res=64, mesh_detail=0).upload(0)
    d_films = alloc_films(sc, dev)
    sc.render_into(*d_films, 0, 4, 21, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    films = tuple(t.cpu().numpy() for t in d_films)
    stats = sc.film_stats_device(*d_films, 4, scale="dB", range=None, bins=256)
    median = float(np.ravel(imageio.percentiles(stats, 50))[0])
    assert np.isfinite(median)
    for kw in ({}, dict(below=False, diagonal=True, min_area=3)):
        got = coverage_holes(sc, d_films, 4, median, **kw)
        assert film_segments_form(sc) == ("global", 0)
        want = coverage_holes(sc, films, 4, median, **kw)
        same_result(got, want, ("holes", kw), plane=got["segments"].cpu().numpy())
        assert got["n_segments"] >= 1 and same_bits(got["threshold"], want["threshold"])
        for k in ("n", "min", "max", "sum"):
            assert same_bits(got["zonal"][k], want["zonal"][k]), k
        assert np.array_equal(got["zonal"]["n"][:, 0], got["area"])
    d_visible = sc.line_of_sight(0, 1, maps=(), ids=("n_visible",))["n_visible"].contiguous()
    d_classes = torch.where(d_visible == 0, 1, -1).to(torch.int32).contiguous()
    classes = d_classes.cpu().numpy().view(np.uint32)
    got = segments(sc, d_classes, min_area=2)
    want = segments(sc, classes, min_area=2)
    same_result(got, want, "shadows", plane=got["segments"].cpu().numpy())
    assert got["n_members"] == int((classes == 1).sum()) > 0 and got["n_segments"] >= 1


def test_segments_between_renders_change_nothing(built):
    """As test_gpu_film_zonal.py's: the call counts nothing and leaves the films alone."""
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import cell_zones
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_films = _to_device(sc, a)
    zones, Z = cell_zones(sc.height, sc.width, 8)
    got = sc.film_segments_device(_d_plane(sc, zones), diagonal=True)
    assert all(v == 0 for v in sc.counters().values()) and got["n_segments"] == Z and got["n_members"] == sc.width * sc.height
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
    from wave_tracer_amd.api import FilmSegmentsInfo, FilmSegmentsSpec, film_segments_form, load_library
    width, height = SHAPES[0]
    sc = segments_scene(tmp_path, width, height)
    dev = torch.device("cuda", 0)
    z = torch.zeros((height, width), dtype=torch.int32, device=dev)
    out = torch.full((height, width), 5, dtype=torch.int32, device=dev)
    with pytest.raises(WtgpuError, match="upload"):
        sc.film_segments_device(z)
    assert film_segments_form(sc) == (None, None)      # no call has launched anything
    lib = load_library()
    info = FilmSegmentsInfo()
    rc = lib.wtgpu_film_segments_device(sc.handle, None, C.byref(FilmSegmentsSpec(0, 1, 0, 0)), z.data_ptr(), None, out.data_ptr(), C.byref(info), None)
    assert rc == 1 and lib.wtgpu_last_error() == b"film_segments: scene not uploaded" and (out == 5).all().item()
    up = scenes[(1, width, height)]
    for bad in (z.long(), z.float(), z[:, :-1], z.cpu(), z.t().contiguous().t()):
        with pytest.raises(ValueError, match="classes: a contiguous torch.int32"):
            up.film_segments_device(bad)
    m = torch.ones((height, width), dtype=torch.float32, device=dev)
    for bad in (m.double(), m[:-1], m.cpu()):
        with pytest.raises(ValueError, match="mask: a contiguous torch.float32"):
            up.film_segments_device(z, mask=bad)
    got = up.film_segments_device(None, mask=m)
    assert (got["n_segments"], got["n_members"], got["area"].tolist()) == (1, width * height, [width * height])
