"""First-hit material maps on the MI355X (wtgpu_first_hit_material, csrc/kernels_firsthit_material.hip) against the host threads
(wtgpu_first_hit_material_host), bit for bit on every float and id: both run csrc/wt/first_hit_material.h — the same rays, the same surface
records, the same material layer, the same sequential f32 sums — in + - x /, comparisons and f32 sqrt under -ffp-contract=off (no test scene
has a function texture with a libm opcode).  Either lane shape (WTGPU_FIRST_HIT_PER_SAMPLE), and the two checks of
tests/test_first_hit_material.py's list that need a device hook: ALBEDO against material_f, channel_wavenumbers against the spectral draw."""
import ctypes as C
import os

import numpy as np
import pytest

from test_first_hit_material import F32, IDS, MAPS, MM, NONE, TEX, same_bits

pytestmark = pytest.mark.gpu


def _device(sc, **kw):
    import torch
    r = sc.first_hit_material(**kw)
    torch.cuda.synchronize(torch.device("cuda", sc.device))
    assert all(v.shape[:2] == (sc.height, sc.width) and v.dtype == (torch.int32 if k in IDS else torch.float32) for k, v in r.items())
    return {k: v.cpu().numpy().view(np.uint32) if k in IDS else v.cpu().numpy() for k, v in r.items()}


def _same(sc, **kw):
    dev, host = _device(sc, **kw), sc.first_hit_material_host(threads=16, **kw)
    assert set(dev) == set(host)
    for k in host:
        a, b = np.ascontiguousarray(dev[k]).view(np.uint32), np.ascontiguousarray(host[k]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (kw, k, int((a != b).sum()), float(np.abs(dev[k].astype(np.float64) - host[k]).max()))
    return dev


@pytest.fixture(scope="module", params=["1", "0"], ids=["per_sample", "per_pixel"])
def scenes(built, request):
    """The scenes, uploaded with either form of the kernel chosen (WTGPU_FIRST_HIT_PER_SAMPLE is read at the upload, and a scene is uploaded
    once): material_maps.xml (37 x 23 = 851 pixels: a last block that is partly empty), textured.xml's five materials at 37 x 37 and
    cornell_box at full tessellation (283 K triangles) at 32 x 32."""
    from wave_tracer_amd import Scene
    old = os.environ.get("WTGPU_FIRST_HIT_PER_SAMPLE")
    os.environ["WTGPU_FIRST_HIT_PER_SAMPLE"] = request.param
    try:
        out = {"mm": Scene.from_xml(MM).upload(0)}
        assert (out["mm"].width * out["mm"].height) % 128 != 0
        for variant in range(1, 6):
            out[f"tex{variant}"] = Scene.from_xml(TEX, defines={"variant": variant}, res=37).upload(0)
        out["box"] = Scene("cornell_box", res=32, mesh_detail=1).upload(0)
        assert out["box"].info.n_tris > 250000
    finally:
        os.environ.pop("WTGPU_FIRST_HIT_PER_SAMPLE") if old is None else os.environ.__setitem__("WTGPU_FIRST_HIT_PER_SAMPLE", old)
    return out


# 0: the centre ray, one lane per pixel; 1: a group narrower than its floats; 7: nine pixels and one idle lane per wavefront; 32: two pixels per
# wavefront; 64: one; 80: more samples than the per-sample form holds, one lane per pixel whatever the knob says
@pytest.mark.parametrize("samples", [0, 1, 7, 32, 64, 80])
def test_device_maps_equal_host(scenes, samples):
    for name, sc in scenes.items():
        k3 = sc.channel_wavenumbers()
        k4 = np.append(k3, F32(2 * np.pi / 500e-6)).astype(F32)      # (500 nm: inside every tabulated IOR of cornell_box)
        full = _same(sc, samples=samples, seed=3, k=k4)            # 20 floats + 2 ids per sample: the whole exchange
        hit = full["material"] != NONE
        assert hit.any() and full["albedo"].shape[-1] == 4, name
        assert name != "mm" or (~hit).any()
        assert (full["material"][hit] < sc.info.n_materials).all() and all(np.isfinite(full[m]).all() for m in MAPS)
        one = _same(sc, samples=samples, seed=3, k=k4[:1], maps=("albedo",), ids=())      # the instantiation without the Fresnel code
        assert same_bits(one["albedo"], full["albedo"][..., :1])
        ids = _same(sc, samples=samples, seed=3, k=k4[:1], maps=(), ids=IDS)
        assert all(same_bits(ids[i], full[i]) for i in IDS)
        two = _same(sc, samples=samples, seed=3, k=k3, maps=("emission", "specular"), ids=("type",))
        assert all(same_bits(two[m], full[m][..., :3]) for m in ("emission", "specular")) and same_bits(two["type"], full["type"])
    assert full["albedo"].any() and scenes["mm"].first_hit_material_host(samples=0)["specular"].any()


def test_python_forms_and_the_guides(built):
    """Scene.first_hit_material's tensors are views of one allocation per group, render.first_hit_material is its numpy form, and
    render.material_guides / join_guides on the device return the host twin's values."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import first_hit_guides, first_hit_material, join_guides, material_guides
    sc = Scene.from_xml(MM)
    r = first_hit_material(sc, samples=7, seed=2)                  # uploads the scene
    host = sc.first_hit_material_host(samples=7, seed=2)
    assert set(r) == set(MAPS) | set(IDS) and all(same_bits(r[n], host[n]) for n in host) and r["type"].dtype == np.uint32
    t = sc.first_hit_material(samples=0, maps=("roughness", "albedo"), ids=IDS)
    assert t["albedo"].shape == (23, 37, 3) and t["albedo"].untyped_storage().data_ptr() == t["roughness"].untyped_storage().data_ptr()
    assert t["material"].untyped_storage().data_ptr() == t["type"].untyped_storage().data_ptr() and t["type"].shape == (23, 37)
    guide, scales, ids = material_guides(sc, samples=7, seed=2)
    hg, hs, _ = material_guides(sc, samples=7, seed=2, host=True)
    assert guide.is_cuda and guide.is_contiguous() and ids is None and scales == hs and same_bits(guide.cpu().numpy(), hg)
    joined, js, jids = join_guides(first_hit_guides(sc), (guide, scales, None))
    assert joined.shape == (23, 37, 8) and joined.is_contiguous() and len(js) == 8 and jids is not None
    assert same_bits(joined[..., 5:].cpu().numpy(), hg)


def test_albedo_is_pi_times_material_f_over_the_cosine(built):
    """ALBEDO on the constant diffuse wall against the BSDF the integrators evaluate: material_f(wi, wo) of a diffuse leaf is wo.z / pi x
    reflectance (Scene.bsdf_queries, the device's material_f), so pi x f / wo.z is the albedo within 4 ulp (two roundings each way)."""
    from wave_tracer_amd import Scene
    sc = Scene.from_xml(MM).upload(0)
    fm = sc.first_hit_material_host(samples=0, maps=("albedo",), ids=("material",))
    wall = sc.first_hit_host(samples=0, maps=(), ids=("shape",))["shape"] == sc.shape_ids.index("r00_diffuse")
    mat, albedo = int(fm["material"][wall][0]), fm["albedo"][wall][0]
    k = sc.channel_wavenumbers()
    wos = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, -0.28, 0.96]], F32)
    q = np.zeros((len(k) * len(wos), 18), np.uint32)
    for j, kj in enumerate(k):
        for i, wo in enumerate(wos):
            row = q[j * len(wos) + i]
            row[0] = mat
            row[1:4] = np.array([0.0, 0.0, 1.0], F32).view(np.uint32)
            row[4:7] = wo.view(np.uint32)
            row[7] = np.array([kj], F32).view(np.uint32)[0]
    f = sc.bsdf_queries(q)[:, 1].copy().view(F32).reshape(len(k), len(wos))
    for j in range(len(k)):
        for i, wo in enumerate(wos):
            got = np.float64(np.pi) * np.float64(f[j, i]) / np.float64(wo[2])
            assert abs(got - np.float64(albedo[j])) <= 4 * np.spacing(albedo[j]), (j, i, got, albedo[j])


def test_channel_wavenumber_of_a_monochromatic_sensor(built):
    """double_slits: the channel's wavenumber is the line, the wavenumber every spectral draw of the scene returns (Scene.source_queries, op 0)."""
    from wave_tracer_amd import Scene
    sc = Scene("double_slits", res=32, lut=(32, 32)).upload(0)
    k = sc.channel_wavenumbers()
    q = np.zeros((8, 24), np.uint32)
    q[:, 15] = 5                                                   # sampler seed
    q[:, 17] = np.arange(8)                                        # sample id
    drawn = sc.source_queries(q)[:, 12].copy().view(F32)
    assert k.shape == (1,) and (drawn == k[0]).all() and k[0] > 0


def test_material_maps_between_renders_change_nothing(built):
    """As test_gpu_first_hit.py::test_first_hit_between_renders_changes_nothing: the maps computed on the device between two renders of the same
    samples leave the counters bit for bit alone and count nothing themselves; the films agree to the order of the renderer's f64 atomic adds."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", res=32, lut=(32, 32)).upload(0)
    m0 = _device(sc, samples=7, seed=6)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    m = _device(sc, samples=7, seed=6)
    assert all(v == 0 for v in sc.counters().values()) and (m["albedo"] > 0).any()
    assert all(same_bits(m[k], m0[k]) for k in m0)
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)


def test_refused_without_an_upload(built):
    import torch
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.api import FirstHitMaterialSpec, _check, load_library
    sc = Scene("cornell_box", res=16, mesh_detail=0)
    with pytest.raises(WtgpuError, match="upload"):
        sc.first_hit_material()
    dev = torch.device("cuda", 0)
    maps, ids = torch.zeros((16, 16, 20), dtype=torch.float32, device=dev), torch.zeros((16, 16, 2), dtype=torch.int32, device=dev)
    spec = FirstHitMaterialSpec(0, 31, 3, 4, (C.c_float * 4)(10000.0, 11000.0, 12000.0, 13000.0), 1)
    with pytest.raises(WtgpuError, match="scene not uploaded"):
        _check(load_library().wtgpu_first_hit_material(sc._h, None, C.byref(spec), maps.data_ptr(), ids.data_ptr()))
    torch.cuda.synchronize(dev)
    assert not maps.any() and not ids.any()
