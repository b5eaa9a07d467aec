"""First-hit maps on the MI355X (wtgpu_first_hit, csrc/kernels_firsthit.hip) against the host threads (wtgpu_first_hit_host), bit for bit: both
run csrc/wt/first_hit.h — the same rays, the same ray queries, the same surface records, the same sequential f32 sums.  The maps use + - x /,
comparisons and f32 sqrt (correctly rounded in the default build) under -ffp-contract=off, so the normals are compared bit for bit too.  And a
call between two renders leaves them alone."""
import ctypes as C
import os

import numpy as np
import pytest

from test_sensor_mask import _write, analytic_xml, masked_radio_xml

pytestmark = pytest.mark.gpu

MAPS = ("coverage", "depth", "position", "normal_geo", "normal_shading", "uv", "facing")
IDS = ("shape", "triangle")
NONE = 0xFFFFFFFF


def _device(sc, **kw):
    import torch
    r = sc.first_hit(**kw)
    torch.cuda.synchronize(torch.device("cuda", sc.device))
    assert all(v.shape[:2] == (sc.height, sc.width) and v.dtype == (torch.int32 if k in IDS else torch.float32) for k, v in r.items())
    return {k: v.cpu().numpy().view(np.uint32) if k in IDS else v.cpu().numpy() for k, v in r.items()}


def _same(sc, **kw):
    dev, host = _device(sc, **kw), sc.first_hit_host(threads=16, **kw)
    assert set(dev) == set(host)
    for k in host:
        a, b = np.ascontiguousarray(dev[k]).view(np.uint32), np.ascontiguousarray(host[k]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (kw, k, int((a != b).sum()), float(np.abs(dev[k].astype(np.float64) - host[k]).max()))
    return dev


@pytest.fixture(scope="module", params=["1", "0"], ids=["per_sample", "per_pixel"])
def scenes(built, tmp_path_factory, request):
    """The four scenes, uploaded with either form of the kernel chosen (WTGPU_FIRST_HIT_PER_SAMPLE is read at the upload, and a scene is uploaded
    once): furnace_path at 37 x 37 (1369 pixels: a last block that is partly empty), the analytic scene (ground rectangles and sky), the radio
    overview at 256 x 192 and cornell_box at full tessellation (283 K triangles)."""
    from wave_tracer_amd import Scene
    tmp = tmp_path_factory.mktemp("gpu_first_hit")
    old = os.environ.get("WTGPU_FIRST_HIT_PER_SAMPLE")
    os.environ["WTGPU_FIRST_HIT_PER_SAMPLE"] = request.param
    try:
        furnace = Scene("furnace_path", res=37, lut=(32, 32)).upload(0)
        assert furnace.info.sensor_type == 0 and (furnace.width * furnace.height) % 128 != 0
        ab = Scene.from_xml(_write(tmp, "ab.xml", analytic_xml())).upload(0)
        radio = Scene.from_xml(_write(tmp, "radio.xml", masked_radio_xml()), defines={"masked_overview": "true"}, res=256).upload(0)
        assert (radio.width, radio.height) == (256, 192)
        box = Scene("cornell_box", res=64, mesh_detail=1).upload(0)
        assert box.info.n_tris > 250000
    finally:
        os.environ.pop("WTGPU_FIRST_HIT_PER_SAMPLE") if old is None else os.environ.__setitem__("WTGPU_FIRST_HIT_PER_SAMPLE", old)
    return {"furnace": furnace, "ab": ab, "radio": radio, "box": box}


# 64: a pixel fills a wavefront; 80: more samples than the per-sample form holds, one lane per pixel whatever the knob says
@pytest.mark.parametrize("samples", [0, 1, 7, 32, 64, 80])
def test_device_maps_equal_host(scenes, samples):
    for name, sc in scenes.items():
        r = _same(sc, samples=samples, seed=3)
        hit = r["coverage"] > 0
        assert hit.any() and np.array_equal(hit, r["shape"] != NONE), name
        assert name not in ("ab", "box") or (~hit).any()      # sky beyond the rectangles; the box is seen from outside
        assert (r["shape"][hit] < sc.info.n_shapes).all() and np.isfinite(r["depth"]).all()
        # the queries that build no surface run another instantiation of the kernel: depth and ids, and every map that needs none
        for maps, ids in ((("depth",), IDS), (("coverage", "depth", "position", "facing"), ())):
            q = _same(sc, samples=samples, seed=3, maps=maps, ids=ids)
            assert all(np.array_equal(q[k].view(np.uint32), r[k].view(np.uint32)) for k in q), (name, maps)
    # a map that needs the surface, alone, and another seed
    _same(scenes["box"], samples=samples, seed=4, maps=("normal_shading",), ids=("triangle",))


def test_first_hit_between_renders_changes_nothing(built):
    """As test_gpu_sensor_mask.py::test_mask_between_renders_changes_nothing: first-hit maps computed on the device between two renders of the
    same samples leave the counters bit for bit alone and count nothing themselves; the films agree to the order of the renderer's f64 atomic
    adds.  Renders do not change the maps either."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    m0 = _device(sc, samples=7, seed=6)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    m = _device(sc, samples=7, seed=6)
    assert all(v == 0 for v in sc.counters().values()) and (m["coverage"] > 0).any()
    assert all(np.array_equal(m[k].view(np.uint32), m0[k].view(np.uint32)) for k in m0)
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)


def test_refused_without_an_upload(built):
    import torch
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.api import FirstHitSpec, _check, load_library
    sc = Scene("cornell_box", res=16, mesh_detail=0)
    with pytest.raises(WtgpuError, match="upload"):
        sc.first_hit()
    dev = torch.device("cuda", 0)
    maps, ids = torch.zeros((16, 16, 14), dtype=torch.float32, device=dev), torch.zeros((16, 16, 2), dtype=torch.int32, device=dev)
    with pytest.raises(WtgpuError, match="scene not uploaded"):
        _check(load_library().wtgpu_first_hit(sc._h, None, C.byref(FirstHitSpec(0, 127, 3, 0, 1)), maps.data_ptr(), ids.data_ptr()))
    torch.cuda.synchronize(dev)
    assert not maps.any() and not ids.any()
    # an uploaded scene: render.first_hit is the numpy form of the same call
    from wave_tracer_amd.render import first_hit
    r = first_hit(sc, samples=0, maps=("depth",), ids=("shape",))
    assert r["depth"].shape == (16, 16) and r["shape"].dtype == np.uint32 and (r["depth"] > 0).any()
    host = sc.first_hit_host(samples=0, maps=("depth",), ids=("shape",))
    assert np.array_equal(r["depth"].view(np.uint32), host["depth"].view(np.uint32)) and np.array_equal(r["shape"], host["shape"])
