"""First-hit maps of a perspective sensor (wtgpu_first_hit_host, csrc/wt/first_hit.h) on the CPU: per pixel the coverage, depth, position,
geometric and shading normal, uv and facing of what its primary rays see first, and the shape and triangle of the first ray that hits.  The
host twin runs the header the device kernel runs (tests/test_gpu_first_hit.py compares them bit for bit)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_sensor_mask import B1, B2, H_CAM, MASK, RES, _footprints, _seq_sum, _write, analytic_xml, masked_radio_xml

HERE = os.path.dirname(os.path.abspath(__file__))
TEX = os.path.join(HERE, "data", "xml", "textured.xml")
NONE = 0xFFFFFFFF
MAPS = ("coverage", "depth", "position", "normal_geo", "normal_shading", "uv", "facing")
IDS = ("shape", "triangle")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def box(built):
    from wave_tracer_amd import Scene
    return Scene("cornell_box", res=32, mesh_detail=0)


@pytest.fixture(scope="module")
def ab(built, tmp_path_factory):
    from wave_tracer_amd import Scene
    return Scene.from_xml(_write(tmp_path_factory.mktemp("first_hit"), "ab.xml", analytic_xml()))


def test_closed_form_on_the_analytic_scene(ab):
    """A camera H_CAM above the origin looks straight down at the rectangles A and B in z = 0, sky beyond B2; one ray through every pixel's
    centre.  The 1e-5 bounds are a few ulps of the operands of the f32 `ro + t rd` (|ro.z| = H_CAM <= depth)."""
    r = ab.first_hit_host(samples=0)
    assert set(r) == set(MAPS + IDS)
    assert all(r[k].shape == (RES, RES) and r[k].dtype == np.float32 for k in ("coverage", "depth", "facing"))
    assert all(r[k].shape == (RES, RES, 3) for k in ("position", "normal_geo", "normal_shading")) and r["uv"].shape == (RES, RES, 2)
    assert all(r[k].shape == (RES, RES) and r[k].dtype == np.uint32 for k in IDS)
    cov = r["coverage"]
    assert np.isin(cov, (0, 1)).all()
    hit = cov == 1
    assert hit.sum() >= 12 * RES and (~hit).sum() >= 8 * RES
    pos, depth = r["position"].astype(np.float64), r["depth"].astype(np.float64)
    assert (np.abs(pos[hit][:, 2]) <= 1e-5 * depth[hit]).all()
    cam = np.array([0.0, 0.0, H_CAM])
    assert np.allclose(depth[hit], np.linalg.norm(pos[hit] - cam, axis=-1), rtol=1e-5, atol=0)
    assert depth[hit].min() >= H_CAM * (1 - 1e-5)
    ng, ns = r["normal_geo"][hit], r["normal_shading"][hit]
    assert np.array_equal(ng, ns)
    assert np.abs(ng[:, :2]).max() <= 1e-6 and np.abs(np.abs(ng[:, 2]) - 1).max() <= 1e-6
    # the camera is above the rectangles: it sees the side their normal points to exactly where that normal points up
    assert np.array_equal(r["facing"][hit] == 1, ng[:, 2] > 0)
    # which way the film's x runs on the ground is read off the positions: one orientation's footprints must hold every pixel centre
    x = pos[..., 0]
    fits = [(x0, x1) for x0, x1 in (_footprints(1), _footprints(-1)) if ((x >= x0) & (x <= x1))[hit].all()]
    assert len(fits) == 1
    x0, x1 = fits[0]
    straddle = ((x0 < B1) & (B1 < x1)) | ((x0 < B2) & (B2 < x1))
    assert straddle.sum() <= 2
    ia, ib = ab.shape_ids.index("A"), ab.shape_ids.index("B")
    sure = hit & ~straddle[None, :]
    assert np.array_equal(r["shape"][sure & (x < B1)], np.full((sure & (x < B1)).sum(), ia, np.uint32)) and (sure & (x < B1)).any()
    over_b = sure & (x > B1) & (x < B2)
    assert (r["shape"][over_b] == ib).all() and over_b.any()
    assert (r["triangle"][hit] < 2).all()                       # a rectangle is two triangles
    assert hit[:, x1 < B2].all() and not hit[:, x0 > B2].any()
    for k in MAPS:
        assert not r[k][~hit].any(), k
    for k in IDS:
        assert (r[k][~hit] == NONE).all(), k


@pytest.mark.parametrize("samples", [1, 7, 32])
def test_same_rays_as_the_mask(ab, box, samples):
    """With no shape flagged the mask counts every hit: it is the sequential f32 sum of 1 / float(samples), taken n_hit times."""
    sums = np.array([_seq_sum(n, samples) for n in range(samples + 1)], np.float32)
    for sc in (ab, box):
        for seed in (3, 11):
            cov = sc.first_hit_host(samples=samples, seed=seed, maps=("coverage",), ids=())["coverage"]
            n = np.round(cov.astype(np.float64) * samples).astype(np.int64)
            assert _same_bits(cov, (n.astype(np.float32) / np.float32(samples)))
            mask = sc.sensor_mask_host(samples=samples, seed=seed, shapes=np.zeros(sc.info.n_shapes))
            assert _same_bits(mask, sums[n])
            assert (n == 0).any() and (n == samples).any() and (samples < 7 or ((n > 0) & (n < samples)).any())


def test_one_sample_sees_the_shape_the_mask_judges(box):
    flags = np.random.default_rng(5).integers(0, 2, box.info.n_shapes)
    assert 0 < flags.sum() < flags.size
    for seed in (1, 2):
        r = box.first_hit_host(samples=1, seed=seed, maps=("coverage",), ids=("shape",))
        mask = box.sensor_mask_host(samples=1, seed=seed, shapes=flags)
        hit = r["coverage"] == 1
        assert np.array_equal(hit, r["shape"] != NONE)
        counted = hit & (flags[np.where(hit, r["shape"], 0)] == 0)
        assert np.array_equal(mask > 0, counted) and counted.any() and (hit & ~counted).any()


def test_subsets_threads_and_seeds(box):
    full = box.first_hit_host(samples=7, seed=4, threads=1)
    # any subset of the bits is, bit for bit, the slices of the full query (queries without normals and uv build no surface: another code path)
    subsets = [((m,), ()) for m in MAPS] + [((), (i,)) for i in IDS] + [((), IDS), (MAPS, ()), (("depth", "position"), IDS),
               (("coverage", "depth", "position", "facing"), ("triangle",)), (("facing", "uv", "coverage"), ("shape",)), (("normal_geo", "depth"), ()),
               (("normal_shading", "position", "facing"), IDS)]
    for maps, ids in subsets:
        r = box.first_hit_host(samples=7, seed=4, maps=maps, ids=ids)
        assert set(r) == set(maps) | set(ids)
        for k, v in r.items():
            assert _same_bits(v, full[k]), (maps, ids, k)
    # the views of one group share one allocation, in bit order whatever order the names come in
    r = box.first_hit_host(samples=7, seed=4, maps=("uv", "depth"), ids=())
    assert r["depth"].base is not None and r["depth"].base is r["uv"].base and r["depth"].base.shape == (32, 32, 3)
    assert _same_bits(r["depth"], r["depth"].base[..., 0])
    five = box.first_hit_host(samples=7, seed=4, threads=5)
    assert all(_same_bits(five[k], full[k]) for k in full)
    other = box.first_hit_host(samples=7, seed=5)
    assert all(not np.array_equal(other[k], full[k]) for k in ("coverage", "depth", "position", "normal_geo", "normal_shading", "uv"))
    a, b = box.first_hit_host(samples=0, seed=4), box.first_hit_host(samples=0, seed=5)
    assert all(_same_bits(a[k], b[k]) for k in a)


def test_means_of_one_and_of_many_samples(box):
    """One sample: the mean is that sample (x / 1.f is x), so normals have unit length and coverage and facing are 0 or 1.  32 samples: a mean of
    unit vectors is no longer than 1, and shorter where the pixel sees an edge (cornell_box has edges between its walls and around its boxes)."""
    one = box.first_hit_host(samples=1, seed=9)
    hit = one["coverage"] == 1
    assert np.isin(one["coverage"], (0, 1)).all() and np.isin(one["facing"], (0, 1)).all() and hit.any()
    for k in ("normal_geo", "normal_shading"):
        length = np.linalg.norm(one[k].astype(np.float64), axis=-1)
        assert np.abs(length[hit] - 1).max() <= 1e-6 and not length[~hit].any()
    many = box.first_hit_host(samples=32, seed=9)
    for k in ("normal_geo", "normal_shading"):
        length = np.linalg.norm(many[k].astype(np.float64), axis=-1)
        assert length.max() <= 1 + 1e-6
        assert (length[many["coverage"] > 0] < 1 - 1e-3).any(), k
    assert ((many["facing"] >= 0) & (many["facing"] <= 1)).all()
    d = many["depth"][many["coverage"] > 0]
    assert d.min() > 0 and np.isfinite(d).all()


def test_uv_and_the_normal_map(built, tmp_path):
    """The textured plane of test_textures.py from above.  Its uv run monotonically across the film.  With a normal map of three texels in a row, the outer ones flat
    ((0.5, 0.5, 1) -> n = (0, 0, 1)) and the middle one tilted, the shading normal is the geometric one, bit for bit, on the flat thirds and
    the tilted one on the middle third; without a normal map the two are equal everywhere.  make_surface's normal-map path is what the map shows."""
    from wave_tracer_amd import Scene
    from wave_tracer_amd.imageio import write_pfm
    tilt = np.array([.3, 0, 1.0]) / np.sqrt(1.09)
    tex = np.array([[[.5, .5, 1.0], (tilt + 1) / 2, [.5, .5, 1.0]]], np.float32)
    write_pfm(str(tmp_path / "n.pfm"), tex)
    nm = Scene.from_xml(TEX, defines={"variant": 4, "bitmap": str(tmp_path / "n.pfm")}).first_hit_host(samples=0)
    plain = Scene.from_xml(TEX, defines={"variant": 1}).first_hit_host(samples=0)
    for r in (nm, plain):
        assert (r["coverage"] == 1).all()
        u, v = r["uv"][..., 0].astype(np.float64), r["uv"][..., 1].astype(np.float64)
        du, dv = np.diff(u, axis=1), np.diff(v, axis=0)
        assert ((du > 0).all() or (du < 0).all()) and ((dv > 0).all() or (dv < 0).all())
        assert np.abs(np.diff(u, axis=0)).max() <= 1e-6 and np.abs(np.diff(v, axis=1)).max() <= 1e-6
        assert 0 < u.min() < u.max() < 1 and 0 < v.min() < v.max() < 1
        assert (np.abs(r["normal_geo"][..., 2]) == 1).all()
    assert _same_bits(plain["normal_shading"], plain["normal_geo"])
    assert _same_bits(nm["normal_geo"], plain["normal_geo"]) and _same_bits(nm["uv"], plain["uv"])
    u = nm["uv"][..., 0]
    differs = (_bits(nm["normal_shading"]) != _bits(nm["normal_geo"])).any(axis=-1)
    assert min(np.abs(u - 1 / 3).min(), np.abs(u - 2 / 3).min()) > 1e-4          # no pixel centre on a seam between two texels
    assert np.array_equal(differs, (u > 1 / 3) & (u < 2 / 3)) and differs.any() and not differs.all()
    t = nm["normal_shading"][differs].astype(np.float64)
    assert np.abs(np.linalg.norm(t, axis=-1) - 1).max() <= 1e-6
    assert np.abs(np.abs(t @ np.array([0, 0, 1.0])) - tilt[2]).max() <= 1e-6     # tilted by the map's angle


def test_normals_to_rgb():
    from wave_tracer_amd.imageio import normals_to_rgb
    n = np.array([[0, 0, 1], [-1, 0, 0], [0, .5, -2], [3, 0, 0]], np.float32)
    assert np.array_equal(normals_to_rgb(n), np.array([[.5, .5, 1], [0, .5, .5], [.5, .75, 0], [1, .5, .5]], np.float32))


def test_errors(box, built, tmp_path):
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.api import FirstHitSpec, _check, load_library
    lib = load_library()
    maps, ids = np.zeros((32, 32, 14), np.float32), np.zeros((32, 32, 2), np.uint32)

    def host(spec, m=maps, i=ids, sc=box):
        _check(lib.wtgpu_first_hit_host(sc._h, C.byref(spec), 1, None if m is None else m.ctypes.data, None if i is None else i.ctypes.data))
    host(FirstHitSpec(0, 127, 3, 0, 1))
    host(FirstHitSpec(4096, 1, 0, 0, 1), i=None)        # a group that is not requested may be NULL; 4096 samples are allowed
    host(FirstHitSpec(0, 0, 2, 0, 1), m=None)
    with pytest.raises(WtgpuError, match="unknown map bits"):
        host(FirstHitSpec(0, 128, 3, 0, 1))
    with pytest.raises(WtgpuError, match="unknown id bits"):
        host(FirstHitSpec(0, 127, 4, 0, 1))
    with pytest.raises(WtgpuError, match="4096 samples"):
        host(FirstHitSpec(4097, 127, 3, 0, 1))
    with pytest.raises(WtgpuError, match="maps pointer is NULL"):
        host(FirstHitSpec(0, 2, 3, 0, 1), m=None)
    with pytest.raises(WtgpuError, match="ids pointer is NULL"):
        host(FirstHitSpec(0, 2, 1, 0, 1), i=None)
    with pytest.raises(WtgpuError, match="nothing requested"):
        host(FirstHitSpec(0, 0, 0, 0, 1))
    with pytest.raises(WtgpuError, match="nothing requested"):
        box.first_hit_host(maps=(), ids=())
    with pytest.raises(ValueError, match="unknown map 'albedo'"):
        box.first_hit_host(maps=("depth", "albedo"))
    with pytest.raises(ValueError, match="unknown id 'material'"):
        box.first_hit_host(ids=("material",))
    # a virtual-plane sensor has no primary ray through a pixel
    vp = Scene.from_xml(_write(tmp_path, "vp.xml", masked_radio_xml(MASK, "virtual_plane")), defines={}, res=32)
    assert vp.info.sensor_type == 1
    with pytest.raises(WtgpuError, match="perspective sensor"):
        vp.first_hit_host()
    # the device call: refused without an upload, before anything touches a device
    with pytest.raises(WtgpuError, match="upload"):
        box.first_hit()
    with pytest.raises(WtgpuError, match="scene not uploaded"):
        _check(lib.wtgpu_first_hit(box._h, None, C.byref(FirstHitSpec(0, 127, 3, 0, 1)), maps.ctypes.data, ids.ctypes.data))
