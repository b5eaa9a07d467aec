"""Line-of-sight maps on the MI355X (wtgpu_line_of_sight, csrc/kernels_los.hip) against the host threads (wtgpu_line_of_sight_host), bit for bit:
both run csrc/wt/los.h — the same points, the same shadow queries, the same sequential f32 sums — with + - x /, comparisons and f32 sqrt
(correctly rounded in the default build) under -ffp-contract=off.  Both forms of the kernel (WTGPU_LOS_PER_SAMPLE), every buffer.  And a call
between two renders leaves them alone."""
import ctypes as C
import os

import numpy as np
import pytest

from test_los import ALL, ELEM, H, IDS, MAPS, NONE, W, los_xml
from test_sensor_mask import _write

pytestmark = pytest.mark.gpu


def _device(sc, **kw):
    import torch
    dev = torch.device("cuda", sc.device)
    args = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if k in ("points", "normals", "mask") and v is not None else v) for k, v in kw.items()}
    r = sc.line_of_sight(**args)
    torch.cuda.synchronize(dev)
    assert all(v.shape[:2] == (sc.height, sc.width) and v.dtype == (torch.int32 if k in IDS else torch.float32) for k, v in r.items())
    return {k: v.cpu().numpy().view(np.uint32) if k in IDS else v.cpu().numpy() for k, v in r.items()}


def _same(sc, **kw):
    dev, host = _device(sc, **kw), sc.line_of_sight_host(threads=16, **kw)
    assert set(dev) == set(host)
    for k in host:
        a, b = np.ascontiguousarray(dev[k]).view(np.uint32), np.ascontiguousarray(host[k]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), ({n: v for n, v in kw.items() if n not in ("points", "normals", "mask")}, k, int((a != b).sum()),
                                                            float(np.abs(dev[k].astype(np.float64) - host[k]).max()))
    return dev


@pytest.fixture(scope="module", params=["1", "0"], ids=["per_sample", "per_pair"])
def scenes(built, tmp_path_factory, request):
    """The three scenes, uploaded with either form of the kernel chosen (WTGPU_LOS_PER_SAMPLE is read at the upload, and a scene is uploaded
    once): the analytic scene of test_los.py at 37 x 23 (851 elements: a last block that is partly empty), the bundled etoile at res 64 (a real
    BVH under a coverage sensor) and cornell_box at res 24 with full tessellation (283 K triangles), whose points come from Scene.first_hit."""
    from wave_tracer_amd import Scene
    tmp = tmp_path_factory.mktemp("gpu_los")
    old = os.environ.get("WTGPU_LOS_PER_SAMPLE")
    os.environ["WTGPU_LOS_PER_SAMPLE"] = request.param
    try:
        plane = Scene.from_xml(_write(tmp, "los.xml", los_xml())).upload(0)
        assert (plane.width, plane.height) == (W, H) and (W * H) % 128 != 0
        etoile = Scene("etoile", res=64, mesh_detail=0).upload(0)
        assert etoile.info.sensor_type == 1
        box = Scene("cornell_box", res=24, mesh_detail=1).upload(0)
        assert box.info.n_tris > 250000
    finally:
        os.environ.pop("WTGPU_LOS_PER_SAMPLE") if old is None else os.environ.__setitem__("WTGPU_LOS_PER_SAMPLE", old)
    return {"plane": plane, "etoile": etoile, "box": box}


@pytest.fixture(scope="module")
def a_mask():
    m = np.ones((H, W), np.float32)
    m[2:9, 5:31], m[12, 0], m[22, 36] = 0, -1, 0
    return m


# 64: an element fills a wavefront; 80: more samples than the per-sample form holds; 0: the centres — both one lane per pair whatever the knob says
@pytest.mark.parametrize("samples", [0, 1, 7, 32, 64, 80])
def test_device_maps_equal_host(scenes, a_mask, samples):
    plane, etoile = scenes["plane"], scenes["etoile"]
    r = _same(plane, samples=samples, seed=3, **ALL)
    assert set(r) == set(MAPS + ELEM + IDS) and (r["visible"][..., 0] == 0).any() and (r["visible"][..., 0] == 1).any() and (r["nearest"] != NONE).all()
    # VISIBLE and the ids alone keep no direction sums: the other instantiation; and every selection size
    q = _same(plane, samples=samples, seed=3, maps=("visible",), ids=IDS)
    assert all(np.array_equal(q[k].view(np.uint32), r[k].view(np.uint32)) for k in q)
    for sel in ([3], [2, 0, 1]):
        q = _same(plane, samples=samples, seed=3, emitters=sel, maps=MAPS, elem=("point",), ids=())
        assert all(np.array_equal(q[k].view(np.uint32), np.ascontiguousarray(r[k][:, :, sel]).view(np.uint32)) for k in MAPS)
    # the mask, without FRONT_ONLY; another seed
    q = _same(plane, samples=samples, seed=4, mask=a_mask, front_only=False, **ALL)
    out = ~(a_mask > 0)
    assert all(not q[k][out].any() for k in MAPS + ELEM + ("n_visible",)) and (q["nearest"][out] == NONE).all() and (q["visible"][~out][:, 2] == 1).all()
    _same(plane, samples=samples, seed=3, mask=a_mask, maps=("distance", "cos"), elem=("nearest_distance",), ids=("nearest",))
    # a real BVH: buildings between the transmitter and the coverage map
    e = _same(etoile, samples=samples, seed=3, **ALL)
    assert (e["visible"] == 0).any() and (e["visible"] == 1).any() and np.isfinite(e["distance"]).all()
    _same(etoile, samples=samples, seed=3, maps=("visible",), ids=("n_visible",))


def test_caller_points_and_an_all_excluding_mask(scenes):
    """cornell_box: the points, normals and mask of Scene.first_hit(samples=0), both lamps; and a mask that excludes every element."""
    import torch
    box, plane = scenes["box"], scenes["plane"]
    fh = box.first_hit(samples=0, maps=("coverage", "position", "normal_geo"), ids=())
    torch.cuda.synchronize(torch.device("cuda", box.device))
    pts, nrm, cov = (fh[k].contiguous().cpu().numpy() for k in ("position", "normal_geo", "coverage"))
    assert (cov > 0).any() and (cov == 0).any()
    for kw in (dict(front_only=False, t_min=1e-3), dict(front_only=True, t_min=1e-3), dict(front_only=False, t_min=0.0)):
        r = _same(box, points=pts, normals=nrm, mask=cov, **ALL, **kw)
        assert (r["visible"] == 1).any() and (r["visible"][cov > 0] == 0).any() and not r["visible"][cov == 0].any()
    _same(box, points=pts, front_only=False, t_min=1e-3, emitters=[1], maps=("visible", "direction"), ids=("n_visible",))
    nothing = np.zeros((H, W), np.float32)
    for samples in (0, 7):
        r = _same(plane, samples=samples, mask=nothing, **ALL)
        assert all(not r[k].any() for k in MAPS + ELEM + ("n_visible",)) and (r["nearest"] == NONE).all()


def test_line_of_sight_between_renders_changes_nothing(built):
    """As test_gpu_first_hit.py::test_first_hit_between_renders_changes_nothing: line-of-sight maps computed on the device between two renders
    of the same samples leave the counters bit for bit alone and count nothing themselves; the films agree to the order of the renderer's f64
    atomic adds.  Renders do not change the maps either."""
    from wave_tracer_amd import Scene, render
    sc = Scene("etoile", res=32, mesh_detail=0).upload(0)
    m0 = _device(sc, samples=7, seed=6, **ALL)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    m = _device(sc, samples=7, seed=6, **ALL)
    assert all(v == 0 for v in sc.counters().values()) and (m["visible"] > 0).any()
    assert all(np.array_equal(m[k].view(np.uint32), m0[k].view(np.uint32)) for k in m0)
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)


def test_refused_without_an_upload(built):
    import torch
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.api import LosSpec, _check, load_library
    from wave_tracer_amd.render import los_masks
    sc = Scene("etoile", res=16, mesh_detail=0)
    with pytest.raises(WtgpuError, match="upload"):
        sc.line_of_sight()
    dev = torch.device("cuda", 0)
    maps, ids = torch.zeros((sc.height, sc.width, 1, 2), dtype=torch.float32, device=dev), torch.zeros((sc.height, sc.width, 2), dtype=torch.int32, device=dev)
    with pytest.raises(WtgpuError, match="scene not uploaded"):
        _check(load_library().wtgpu_line_of_sight(sc._h, None, C.byref(LosSpec(0, 3, 0, 3, 1, 0, (C.c_uint32 * 32)(), 0.0, 0, 1)), None, None, None,
                                                  maps.data_ptr(), None, ids.data_ptr()))
    torch.cuda.synchronize(dev)
    assert not maps.any() and not ids.any()
    # an uploaded scene: the masks of the film passes, on the device, equal the host's
    sc.upload(0)
    los, nlos = los_masks(sc, samples=7, seed=2)
    torch.cuda.synchronize(dev)
    assert los.is_cuda and los.dtype == torch.float32 and tuple(los.shape) == (sc.height, sc.width) and float((los + nlos).sum()) == sc.width * sc.height
    host = los_masks(sc, samples=7, seed=2, host=True)
    assert np.array_equal(los.cpu().numpy(), host[0]) and np.array_equal(nlos.cpu().numpy(), host[1]) and 0 < host[0].sum() < host[0].size
