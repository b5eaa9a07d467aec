"""By-geometry sensor masks on the MI355X (wtgpu_sensor_mask, csrc/kernels_mask.hip) against the host threads (wtgpu_sensor_mask_host), bit for
bit: the same draws, the same ray queries, the same sequential f32 sums.  And a mask computed between two renders leaves them alone."""
import numpy as np
import pytest

from test_sensor_mask import _write, analytic_xml, masked_radio_xml

pytestmark = pytest.mark.gpu


def _device_mask(sc, **kw):
    import torch
    m = sc.sensor_mask(**kw)
    torch.cuda.synchronize(m.device)
    assert m.shape == (sc.height, sc.width) and m.dtype == torch.float32
    return m.cpu().numpy()


def _same(sc, **kw):
    dev, host = _device_mask(sc, **kw), sc.sensor_mask_host(threads=16, **kw)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (kw, int((dev != host).sum()))
    return dev


@pytest.mark.parametrize("samples", [32, 7, 1, 64])   # (1: sixty-four pixels per wavefront; 64: the wavefront is one pixel)
def test_device_mask_equals_host(built, tmp_path, samples):
    from wave_tracer_amd import Scene
    # the analytic scene: ground rectangles A (matches) and B, sky beyond
    ab = Scene.from_xml(_write(tmp_path, "ab.xml", analytic_xml())).upload(0)
    for seed in (1, 2):
        m = _same(ab, samples=samples, seed=seed)
        assert (m == 0).any() and (m > 0).any()
    # the masked radio overview at 256 x 192: the scene file's flags
    radio = Scene.from_xml(_write(tmp_path, "radio.xml", masked_radio_xml()), defines={"masked_overview": "true"}, res=256).upload(0)
    assert (radio.width, radio.height) == (256, 192)
    m = _same(radio, samples=samples, seed=3)
    assert (m == 0).any() and (m > 0).any()
    # cornell_box at full tessellation (283 K triangles), flags from the caller
    box = Scene("cornell_box", res=128, mesh_detail=1).upload(0)
    assert box.info.n_tris > 250000
    flags = np.arange(box.info.n_shapes) % 2
    m = _same(box, samples=samples, seed=4, shapes=flags)
    assert 0 < (m > 0).mean() < 1


def test_per_lane_form_beyond_64_samples(built, tmp_path):
    """More than 64 samples per pixel do not fit one wavefront's ballot: one lane per pixel, same values."""
    from wave_tracer_amd import Scene
    ab = Scene.from_xml(_write(tmp_path, "ab.xml", analytic_xml())).upload(0)
    m = _same(ab, samples=80, seed=9)
    assert (m == 0).any() and (m > 0).any()


def test_mask_between_renders_changes_nothing(built):
    """A mask computed on the device between two renders of the same samples leaves the counters bit for bit alone and counts nothing itself;
    the films agree to the order of the renderer's f64 atomic adds (two renders differ by that much without any mask in between:
    test_gpu_render.py::test_sample_range_additivity_and_determinism).  Renders do not change the mask either."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    assert sc.info.sensor_type == 0
    flags = np.zeros(sc.info.n_shapes)
    m0 = _device_mask(sc, shapes=flags, seed=6)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    m = _device_mask(sc, shapes=flags, seed=6)
    assert all(v == 0 for v in sc.counters().values()) and (m > 0).any() and np.array_equal(m, m0)
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
