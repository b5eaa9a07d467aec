"""First-hit material maps (wtgpu_first_hit_material_host, Scene.first_hit_material_host, Scene.channel_wavenumbers, render.material_guides,
render.join_guides) on the CPU: the host twin against closed forms on tests/data/xml/material_maps.xml and tests/data/xml/textured.xml, an f64
numpy Fresnel, the first-hit maps of the same rays, and itself (subsets, wavenumber counts, threads, seeds).  The device is held to the host
twin bit for bit in tests/test_gpu_first_hit_material.py, where the two checks that need a device hook (Scene.bsdf_queries, Scene.source_queries)
stand too.  Measured figures: tests/golden/first_hit_material_measured.json; a tolerance there is 10 x the measurement, the project's rule."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MM = os.path.join(HERE, "data", "xml", "material_maps.xml")
TEX = os.path.join(HERE, "data", "xml", "textured.xml")
MEASURED = json.load(open(os.path.join(HERE, "golden", "first_hit_material_measured.json")))
F32 = np.float32
NONE = 0xFFFFFFFF
MAPS = ("albedo", "specular", "opacity", "roughness", "emission")
IDS = ("material", "type")
RGB4 = np.array([[[0.2, 0.2, 0.9], [0.5, 0.5, 0.5]], [[0.8, 0.3, 0.1], [0.1, 0.6, 0.2]]], F32)   # tests/golden/first_hit_material_rgb4.pfm, rows from the image's top


def k_of_nm(nm):
    return F32(2 * np.pi / (nm * 1e-6))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def mm(built):
    from wave_tracer_amd import Scene
    return Scene.from_xml(MM)


@pytest.fixture(scope="module")
def mm0(mm):
    """the centre-ray queries every closed form reads, computed once: (first-hit maps, material maps at the channel wavenumbers, pixels by shape id)"""
    fh = mm.first_hit_host(samples=0)
    fm = mm.first_hit_material_host(samples=0)
    pix = {name: fh["shape"] == i for i, name in enumerate(mm.shape_ids)}
    assert all(p.sum() >= 8 for p in pix.values()), {n: int(p.sum()) for n, p in pix.items()}
    return fh, fm, pix


def textured(variant):
    from wave_tracer_amd import Scene
    return Scene.from_xml(TEX, defines={"variant": variant}, res=37)


def checker_parity(uv):
    """1 where the 4 x 4 checker of textured.xml / material_maps.xml shows its first colour: floor(4u) and floor(4v) of equal parity"""
    c = (F32(4) * uv).astype(np.int32)
    return (c[..., 0] % 2) == (c[..., 1] % 2)


def rgb_uplift(r, g, b, k):
    """wt/scene.h's rgb_uplift restated in numpy f32, operation by operation"""
    tab = {n: np.array(v, F32) for n, v in dict(
        white=[1.0000, 1.0000, 0.9999, 0.9993, 0.9992, 0.9998, 1.0000, 1.0000, 1.0000, 1.0000],
        cyan=[0.9710, 0.9426, 1.0007, 1.0007, 1.0007, 1.0007, 0.1564, 0.0000, 0.0000, 0.0000],
        magenta=[1.0000, 1.0000, 0.968, 0.22295, 0.0000, 0.0458, 0.8369, 1.0000, 1.0000, 0.9959],
        yellow=[0.0001, 0.0000, 0.1088, 0.6651, 1.0000, 1.0000, 0.9996, 0.9586, 0.9685, 0.9840],
        red=[0.1012, 0.0515, 0.0000, 0.0000, 0.0000, 0.0000, 0.8325, 1.0149, 1.0149, 1.014],
        green=[0.0000, 0.0000, 0.0273, 0.7937, 1.0000, 0.9418, 0.1719, 0.0000, 0.0000, 0.0025],
        blue=[1.0000, 1.0000, 0.8916, 0.3323, 0.0000, 0.0000, 0.0003, 0.0369, 0.0483, 0.0496]).items()}
    r, g, b, k = F32(r), F32(g), F32(b), F32(k)
    lam = F32(6.2831853) / k * F32(1e6)
    if not (380 <= lam <= 720):
        return F32(0)
    i = int((lam - F32(380)) / (F32(720) - F32(380)) * F32(10))
    if i > 9:
        return F32(0)
    if r <= g and r <= b:
        terms = [("white", r)] + ([("cyan", g - r), ("blue", b - g)] if g <= b else [("cyan", b - r), ("green", g - b)])
    elif g <= r and g <= b:
        terms = [("white", g)] + ([("magenta", r - g), ("blue", b - r)] if r <= b else [("magenta", b - g), ("red", r - b)])
    else:
        terms = [("white", b)] + ([("yellow", r - b), ("green", g - r)] if r <= g else [("yellow", g - b), ("red", r - g)])
    total = F32(0)
    for name, x in terms:
        total = F32(total + F32(tab[name][i] * F32(x)))
    return total


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def test_textured_plane_checker_scale_wrapper_and_mask(built):
    """textured.xml at 37 x 37, centre rays: the checker's albedo is exactly 0.8f / 0.2f by the parity of floor(4u), floor(4v) of first_hit_host's
    uv, as a reflectance texture (variant 1) and as the factor of a scale wrapper over a white wall (variant 5); the checker as a mask (variant
    3) gives OPACITY 1 / 0 and ALBEDO 0.5f x OPACITY.  Nothing else is set: no specular, no roughness, no emission, every leaf diffuse."""
    for variant in (1, 5, 3):
        sc = textured(variant)
        uv = sc.first_hit_host(samples=0, maps=("uv",), ids=())["uv"]
        fm = sc.first_hit_material_host(samples=0)
        first = checker_parity(uv)
        assert first.any() and (~first).any() and fm["albedo"].shape == (37, 37, 3)
        if variant == 3:
            exp_a, exp_o = np.where(first, F32(0.5), F32(0)), np.where(first, F32(1), F32(0))
        else:
            exp_a, exp_o = np.where(first, F32(0.8), F32(0.2)), np.ones((37, 37), F32)
        for j in range(3):
            assert same_bits(fm["albedo"][..., j], exp_a) and same_bits(fm["opacity"][..., j], exp_o), (variant, j)
        assert not fm["specular"].any() and not fm["roughness"].any() and not fm["emission"].any()
        assert (fm["type"] == 0).all() and (fm["material"] != NONE).all()


def test_material_maps_closed_forms(mm, mm0):
    fh, fm, pix = mm0
    k = mm.channel_wavenumbers()
    one, zero = F32(1), F32(0)

    def expect(shape, **maps):
        p = pix[shape]
        for name in MAPS:
            got = fm[name][p]                                            # [n, 3]
            want = np.asarray(maps.get(name, zero), F32)                 # one value, one per pixel, or one per pixel and wavenumber
            want = np.broadcast_to(want[:, None] if want.ndim == 1 else want, got.shape)
            assert same_bits(got, want), (shape, name, got[:2], want[:2])

    expect("r00_diffuse", albedo=F32(0.5), opacity=one)
    expect("r01_behind", opacity=one)                                    # one-sided, seen from behind: wi.z < 0
    expect("r02_mask", albedo=F32(0.8) * F32(0.6), opacity=F32(0.6))
    expect("r03_composite", albedo=F32(0.7), opacity=one)                # (the reader keeps the visible bin: see the scene file)
    expect("r04_scale", albedo=F32(0.6) * F32(0.5), opacity=one)
    expect("r06_conductor", specular=fm["specular"][pix["r06_conductor"]], opacity=one, roughness=F32(0.3))
    rough = np.where(checker_parity(fh["uv"][pix["r07_rough_tex"]]), F32(0.1) + F32(0.4) * one, F32(0.1) + F32(0.4) * zero)
    assert len(set(rough.tolist())) == 2
    expect("r07_rough_tex", specular=fm["specular"][pix["r07_rough_tex"]], opacity=one, roughness=rough)
    expect("r05_dielectric", specular=fm["specular"][pix["r05_dielectric"]], opacity=one)
    v = fh["uv"][pix["r09_function"]][:, 1]
    fn = np.where(v > F32(0.5), F32(0.3) + F32(0.5) * v, F32(0.2)).astype(F32)     # mix(0.2, 0.3 + 0.5 v, v > 0.5)
    assert (v > 0.5).any() and (v <= 0.5).any()
    expect("r09_function", albedo=fn, opacity=one)
    expect("r10_emitter", albedo=F32(0.25), opacity=one, emission=F32(3) * F32(0.25))
    expect("r11_emitter_away", opacity=one)
    # the RGB bitmap, nearest texel: uv (0, 0) is the image's bottom-left corner
    p = pix["r08_rgb"]
    uv, got = fh["uv"][p], fm["albedo"][p]
    texels = set()
    for (u, v), g in zip(uv, got):
        col, row = int(u >= 0.5), int(v < 0.5)
        texels.add((col, row))
        want = np.array([min(one, max(zero, rgb_uplift(*RGB4[row, col], kj))) for kj in k], F32)
        assert same_bits(g, want), (u, v, g, want)
    assert len(texels) == 4
    assert not fm["specular"][p].any() and same_bits(fm["opacity"][p], np.ones_like(got))
    # ids: the material is the shape's, the type the leaf's; the background holds 0xFFFFFFFF and zeros
    leaf = {"r05_dielectric": 1, "r06_conductor": 2, "r07_rough_tex": 2}
    for name, p in pix.items():
        assert (fm["type"][p] == leaf.get(name, 0)).all(), name
        assert len(set(fm["material"][p].tolist())) == 1 and fm["material"][p][0] != NONE
    assert len({int(fm["material"][p][0]) for p in pix.values()}) == len(pix)
    miss = fh["shape"] == NONE
    assert miss.any() and (fm["material"][miss] == NONE).all() and (fm["type"][miss] == NONE).all()
    assert all(not fm[name][miss].any() for name in MAPS)


@pytest.mark.parametrize("wall", ["composite", "composite_gap"])
def test_composite_bins_at_run_time(built, wall):
    """The bundled furnace with a composite wall (bins 300 .. 550 nm -> diffuse 0.8 and, without the gap, 550 .. 800 nm -> diffuse 0.2): one
    wavenumber in each bin gives each bin's albedo, a wavenumber in the gap gives 0 in every float, and TYPE reads 0xFFFFFFFF when k[0] is there."""
    from wave_tracer_amd import Scene
    sc = Scene("furnace_wall_" + wall, res=24)
    fm = sc.first_hit_material_host(samples=0, k=[k_of_nm(450), k_of_nm(650)])
    walls = fm["albedo"][..., 0] == F32(0.8)
    assert walls.mean() > 0.5
    assert (fm["albedo"][..., 1][walls] == (F32(0.2) if wall == "composite" else F32(0))).all()
    assert (fm["opacity"][..., 1][walls] == (1 if wall == "composite" else 0)).all() and (fm["opacity"][..., 0][walls] == 1).all()
    assert (fm["type"][walls] == 0).all()
    back = sc.first_hit_material_host(samples=0, k=[k_of_nm(650), k_of_nm(450)])
    assert same_bits(back["albedo"][..., 0], fm["albedo"][..., 1]) and same_bits(back["albedo"][..., 1], fm["albedo"][..., 0])
    assert same_bits(back["material"], fm["material"])
    assert (back["type"][walls] == (0 if wall == "composite" else NONE)).all()


def fresnel_f64(eta, cos_i):
    """the unpolarised power reflectance of a smooth interface of relative index eta = n_outside / n_inside (complex), f64"""
    eta, c = np.complex128(eta), np.asarray(cos_i, np.float64)
    t = np.sqrt(1 - (1 - c ** 2) * eta ** 2)
    rs, rp = (eta * c - t) / (eta * c + t), (c - eta * t) / (c + eta * t)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


def test_specular_against_an_f64_fresnel(built, mm0):
    """SPECULAR on the dielectric (the transmitting branch: 1 - (Ts + Tp) / 2 at the real index) and on the conductor (the complex branch) against
    the f64 Fresnel equations at each pixel's own incidence, cos = dot(-d, shading normal) from first_hit_host's position and normal: from the
    scene's own camera (cos 0.99 .. 1) and from one 14 m to the side (-Dcamx=14: cos 0.55 .. 0.65).  Measured here, the largest difference:
    dielectric 1.7e-7, conductor 6.7e-7; at the pixel nearest normal incidence (cos 0.99973) the dielectric is 0.04 within 3.8e-8, held to the
    dielectric's bound.  The bounds are 10 x what tests/golden/first_hit_material_measured.json holds."""
    from wave_tracer_amd import Scene
    worst = {}
    for camx in (0, 14):
        if camx:
            sc = Scene.from_xml(MM, defines={"camx": camx})
            fh, fm = sc.first_hit_host(samples=0), sc.first_hit_material_host(samples=0, maps=("specular",), ids=())
            pix = {name: fh["shape"] == i for i, name in enumerate(sc.shape_ids)}
        else:
            fh, fm, pix = mm0
        for shape, eta in (("r05_dielectric", 1 / 1.5), ("r06_conductor", 1 / (1.2 + 4j))):
            p = pix[shape]
            d = fh["position"][p].astype(np.float64) - np.array([camx, 0.0, 10.5])
            cos_i = -(d / np.linalg.norm(d, axis=-1, keepdims=True) * fh["normal_shading"][p].astype(np.float64)).sum(-1)
            assert p.sum() >= 4 and (((cos_i > 0.5) & (cos_i < 0.7)).all() if camx else (cos_i > 0.99).all())
            ref = fresnel_f64(eta, cos_i)
            for j in range(3):
                worst[shape] = max(worst.get(shape, 0.0), float(np.abs(fm["specular"][p][:, j] - ref).max()))
            if shape == "r05_dielectric" and not camx:
                nearest = np.argmax(cos_i)
                at_normal = abs(float(fm["specular"][p][nearest, 0]) - 0.04)
                print(f"first_hit_material: dielectric at cos {cos_i[nearest]:.6f}: |specular - 0.04| = {at_normal:.3e}")
                assert at_normal <= 10 * MEASURED["specular_max_abs_diff"]["r05_dielectric"]
    print("first_hit_material: specular, largest difference from the f64 Fresnel:", worst)
    for shape, w in worst.items():
        assert w <= 10 * MEASURED["specular_max_abs_diff"][shape], (shape, w)


# ---- consistency ---------------------------------------------------------------------------------------------------------------------------
def test_hit_set_and_material_per_shape(mm):
    for samples, seed in ((0, 1), (7, 3), (32, 5)):
        fh = mm.first_hit_host(samples=samples, seed=seed, maps=(), ids=("shape",))
        fm = mm.first_hit_material_host(samples=samples, seed=seed, maps=(), ids=IDS)
        assert np.array_equal(fm["material"] != NONE, fh["shape"] != NONE)
        for s in range(len(mm.shape_ids)):
            assert len(set(fm["material"][fh["shape"] == s].tolist())) <= 1


def test_subsets_wavenumber_counts_threads(mm):
    k4 = np.append(mm.channel_wavenumbers(), k_of_nm(900)).astype(F32)        # (900 nm: outside the RGB uplift, inside every constant spectrum)
    full = mm.first_hit_material_host(samples=7, seed=4, k=k4, threads=1)
    assert set(full) == set(MAPS) | set(IDS) and full["albedo"].shape == (23, 37, 4) and full["type"].shape == (23, 37)
    for bits in range(1, 32):
        maps = tuple(n for i, n in enumerate(MAPS) if bits >> i & 1)
        for ids in ((), ("material",), ("type",), IDS) if bits in (1, 2, 9, 21, 31) else (IDS if bits % 2 else (),):
            r = mm.first_hit_material_host(samples=7, seed=4, k=k4, maps=maps, ids=ids)
            assert set(r) == set(maps) | set(ids)
            assert all(same_bits(v, full[n]) for n, v in r.items()), (maps, ids)
    for ids in (("material",), ("type",), IDS):
        r = mm.first_hit_material_host(samples=7, seed=4, k=k4, maps=(), ids=ids)
        assert set(r) == set(ids) and all(same_bits(v, full[n]) for n, v in r.items())
    # the views of one group share one allocation, in bit order whatever order the names come in
    r = mm.first_hit_material_host(samples=7, seed=4, k=k4, maps=("emission", "albedo"), ids=())
    assert r["albedo"].base is r["emission"].base and r["albedo"].base.shape == (23, 37, 8) and same_bits(r["emission"], r["albedo"].base[..., 4:])
    for n_k in (1, 2, 3):
        r = mm.first_hit_material_host(samples=7, seed=4, k=k4[:n_k])
        assert all(same_bits(r[n], full[n][..., :n_k]) for n in MAPS) and all(same_bits(r[n], full[n]) for n in IDS), n_k
    five = mm.first_hit_material_host(samples=7, seed=4, k=k4, threads=5)
    assert all(same_bits(five[n], full[n]) for n in full)
    # at 900 nm the RGB bitmap's uplift is 0 and every constant reflectance is what it is in the visible
    rgb = mm.first_hit_host(samples=0, maps=(), ids=("shape",))["shape"] == mm.shape_ids.index("r08_rgb")
    c = mm.first_hit_material_host(samples=0, k=k4, maps=("albedo",), ids=())["albedo"]
    assert not c[rgb][:, 3].any() and c[rgb][:, :3].all() and same_bits(c[~rgb][:, 3], c[~rgb][:, 0])


def interior(shape):
    """pixels whose 3 x 3 neighbourhood shows one shape (or nothing) to the centre rays: every sample of such a pixel sees what its centre sees"""
    H, W = shape.shape
    pad = np.pad(shape, 1, mode="edge")
    same = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            same &= pad[dy:dy + H, dx:dx + W] == shape
    return same


def test_sample_counts_means_and_seeds(mm, mm0):
    fh, fm0, pix = mm0
    const = np.zeros_like(pix["r00_diffuse"])
    for name in ("r00_diffuse", "r01_behind", "r02_mask", "r03_composite", "r04_scale", "r10_emitter", "r11_emitter_away"):
        const |= pix[name]
    inner = interior(fh["shape"])
    inside = inner & const
    assert inside.sum() >= 20 and (inner & (fh["shape"] == NONE)).any()
    # one sample: the mean is that sample (x / 1.f is x) — on the textured plane the checker's own two values at that sample's uv
    sc = textured(1)
    uv = sc.first_hit_host(samples=1, seed=9, maps=("uv",), ids=())["uv"]
    one = sc.first_hit_material_host(samples=1, seed=9, maps=("albedo",), ids=())["albedo"]
    assert same_bits(one[..., 0], np.where(checker_parity(uv), F32(0.8), F32(0.2)))
    assert not same_bits(uv, sc.first_hit_host(samples=0, maps=("uv",), ids=())["uv"])
    # many samples: a sequential f32 sum in sample order, divided once by float(n_hit) — restated where every sample sees one value
    for samples in (7, 32):
        fm = mm.first_hit_material_host(samples=samples, seed=9)
        for name in ("albedo", "opacity", "emission"):
            x = fm0[name][inside]
            total = np.zeros_like(x)
            for _ in range(samples):
                total = (total + x).astype(F32)
            assert same_bits(fm[name][inside], (total / F32(samples)).astype(F32)), (samples, name)
        assert same_bits(fm["material"][inner], fm0["material"][inner])
    m32 = mm.first_hit_material_host(samples=32, seed=9, maps=("albedo",), ids=())["albedo"]
    x = F32(0.8) * F32(0.6)
    total = F32(0)
    for _ in range(32):
        total = F32(total + x)
    assert total / F32(32) != x, "the case tells a sequential sum from a tree of doublings"
    assert (m32[inner & pix["r02_mask"]] == total / F32(32)).all()
    # two seeds differ, and only where a pixel sees an edge or a texture
    a, b = (mm.first_hit_material_host(samples=7, seed=s) for s in (4, 5))
    differ = np.zeros_like(const)
    for name in MAPS:
        differ |= (a[name].view(np.uint32) != b[name].view(np.uint32)).any(-1)
    assert differ.any() and not (differ & (inside | (inner & (fh["shape"] == NONE)))).any()
    a, b = (mm.first_hit_material_host(samples=0, seed=s) for s in (4, 5))
    assert all(same_bits(a[n], b[n]) for n in a)


# ---- channel wavenumbers -----------------------------------------------------------------------------------------------------------------
def test_channel_wavenumbers_of_an_rgb_sensor(mm):
    """Python cannot read the response tables, so only properties are checked: one wavenumber per channel, each inside the visible band, red's
    wavelength above green's above blue's.  (The monochromatic case stands in the GPU file: it needs Scene.source_queries.)"""
    k = mm.channel_wavenumbers()
    assert k.dtype == np.float32 and k.shape == (3,)
    lam = 2 * np.pi / k.astype(np.float64) * 1e6
    assert ((lam > 380) & (lam < 720)).all() and lam[0] > lam[1] > lam[2]
    from wave_tracer_amd import Scene
    mono = Scene("double_slits", res=32, lut=(32, 32)).channel_wavenumbers()
    assert mono.shape == (1,) and np.isfinite(mono[0]) and mono[0] > 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(mm):
    import ctypes as C
    from wave_tracer_amd import Scene, WtgpuError
    from wave_tracer_amd.api import FirstHitMaterialSpec, load_library
    lib = load_library()
    k = (C.c_float * 4)(10000.0, 10000.0, 10000.0, 10000.0)
    maps, ids = np.zeros((23, 37, 20), F32), np.zeros((23, 37, 2), np.uint32)

    def call(spec, m=maps, i=ids, scene=mm):
        rc = lib.wtgpu_first_hit_material_host(scene._h, C.byref(spec), 1, None if m is None else m.ctypes.data, None if i is None else i.ctypes.data)
        lib.wtgpu_last_error.restype = C.c_char_p
        return rc, lib.wtgpu_last_error().decode()

    def spec(samples=0, maps=31, ids=3, n_k=1, kk=k):
        return FirstHitMaterialSpec(samples, maps, ids, n_k, kk, 1)

    for sp, kw, msg in ((spec(maps=32), {}, "unknown map bits"), (spec(ids=4), {}, "unknown id bits"), (spec(n_k=0), {}, "1 .. 4 wavenumbers"),
                        (spec(n_k=5), {}, "1 .. 4 wavenumbers"), (spec(samples=4097), {}, "0 .. 4096 samples"), (spec(maps=0, ids=0), {}, "nothing requested"),
                        (spec(), {"m": None}, "maps pointer is NULL"), (spec(), {"i": None}, "ids pointer is NULL")):
        rc, text = call(sp, **kw)
        assert rc != 0 and msg in text, (msg, text)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, text = call(spec(n_k=2, kk=(C.c_float * 4)(10000.0, bad, 1.0, 1.0)))
        assert rc != 0 and "wavenumber 1 is not finite and > 0" in text, (bad, text)
    assert call(spec(maps=1, ids=0), i=None)[0] == 0 and call(spec(maps=0, ids=1), m=None)[0] == 0      # a group that is not requested may be NULL
    with pytest.raises(ValueError, match="unknown map 'colour'"):
        mm.first_hit_material_host(maps=("colour",))
    with pytest.raises(WtgpuError, match="1 .. 4 wavenumbers"):
        mm.first_hit_material_host(k=[1.0, 2.0, 3.0, 4.0, 5.0])
    with pytest.raises(WtgpuError, match="upload"):
        mm.first_hit_material()
    vp = Scene("double_slits", res=32, lut=(32, 32))                       # a virtual-plane sensor
    with pytest.raises(WtgpuError, match="need a perspective sensor"):
        vp.first_hit_material_host()


# ---- guides --------------------------------------------------------------------------------------------------------------------------------
def test_material_guides_and_join_guides(mm, mm0):
    from wave_tracer_amd.render import MATERIAL_GUIDE_SCALE, first_hit_guides, join_guides, material_guides, shadow_guides
    fh, fm, pix = mm0
    guide, scales, ids = material_guides(mm, host=True)
    assert guide.shape == (23, 37, 3) and guide.dtype == np.float32 and guide.flags.c_contiguous and ids is None
    assert scales == [MATERIAL_GUIDE_SCALE] * 3 and abs(MATERIAL_GUIDE_SCALE - 2.78) < 0.005
    total = fm["albedo"] + fm["specular"] + fm["emission"]
    assert same_bits(guide, np.clip(total, 0, 1)) and guide.max() == 1
    assert (total[pix["r10_emitter"]] == F32(0.25) + F32(0.75)).all()
    g7, s7, _ = material_guides(mm, samples=7, seed=3, scales=[1, 2, 3], host=True)
    assert s7 == [1.0, 2.0, 3.0] and not same_bits(g7, guide)
    geo = first_hit_guides(mm, host=True)
    joined, js, jids = join_guides(geo, (guide, scales, ids))
    assert joined.shape == (23, 37, 8) and joined.flags.c_contiguous and js == geo[1] + scales and jids is geo[2]
    assert same_bits(joined[..., :5], geo[0]) and same_bits(joined[..., 5:], guide)
    j2, s2, i2 = join_guides((guide, scales, None), (guide[..., 0], [4.0], None), (None, [], geo[2]))
    assert j2.shape == (23, 37, 4) and s2 == scales + [4.0] and i2 is geo[2]
    with pytest.raises(ValueError, match="at most 8"):
        join_guides(geo, (guide, scales, None), (guide[..., :1], [1.0], None))
    with pytest.raises(ValueError, match="planes with"):
        join_guides((guide, [1.0], None))


def test_quality_of_the_albedo_guide_on_a_checker_weaker_than_the_noise(built):
    """textured.xml variant 1 at 37 x 37, host twins only.  Two half-films: the host ALBEDO scaled to a contrast of 0.08 around 0.5 plus independent
    Gaussian noise of sigma 0.1 per half (the figures of the guided filter's own quality test), three seeds; denoised with window 5 and patch 2.
    The yardsticks are the parent's calls on the same films: the unguided filter and first_hit_guides, whose planes are constant across the flat
    wall.  RMSE against the noise-free pattern, measured here (unguided / first_hit_guides / material_guides):
    seed 0: 0.027992 / 0.027992 / 0.022250;  seed 1: 0.029527 / 0.029527 / 0.023335;  seed 2: 0.029506 / 0.029506 / 0.022002
    — the values of tests/golden/first_hit_material_measured.json; no ratio was fixed in advance."""
    from wave_tracer_amd.render import denoise, first_hit_guides, material_guides
    sc = textured(1)
    albedo = sc.first_hit_material_host(samples=0, maps=("albedo",), ids=())["albedo"].astype(np.float64)
    truth = 0.5 + 0.08 * (albedo - 0.5) / 0.3
    assert set(np.round(truth, 6).ravel().tolist()) == {0.42, 0.58}
    H, W, _ = truth.shape
    geo, mat = first_hit_guides(sc, host=True), material_guides(sc, host=True)
    rms = lambda t: float(np.sqrt((t ** 2).mean()))
    for seed in range(3):
        rng = np.random.default_rng(seed)
        a, b = (((truth + 0.1 * rng.normal(size=truth.shape)).astype(F32).astype(np.float64), np.ones((H, W)), np.zeros((H, W, 3))) for _ in range(2))
        got = {}
        for name, guides in (("unguided", None), ("first_hit_guides", geo), ("material_guides", mat)):
            film = denoise(sc, a, b, 1, guides=guides, window=5, patch=2)["film"].reshape(H, W, 3).astype(np.float64)
            got[name] = rms(film - truth)
        print(f"first_hit_material quality seed {seed}: " + " ".join(f"{n} {v:.6f}" for n, v in got.items()), "; recorded", MEASURED["quality_rmse"][seed])
        assert got["material_guides"] < got["unguided"] and got["material_guides"] < got["first_hit_guides"], got
