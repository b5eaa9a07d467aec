"""By-geometry sensor masks (include/wt/sensor/mask/mask.hpp, src/sensor/mask.cpp:28-108) on the CPU: the scene reader's <sensor_mask>, the
shape ids, and the mask itself through wtgpu_sensor_mask_host (the reference's own CPU job; tests/test_gpu_sensor_mask.py compares the device
against it).  A mask value is the share of a pixel's `samples` primary rays whose first hit is on a shape whose id does NOT match the regex."""
import math
import os

import numpy as np
import pytest

from test_xml_scene import _radio_city_xml

MASK = r'<sensor_mask type="by-geometry"><string name="mask_id_regex" value="^mesh-Plane\$"/></sensor_mask>'
REF_ETOILE = "/root/reference/scenes/sionna_etoile/etoile.xml"


COVERAGE_ON = '<sensor type="virtual_plane" id="coverage"><boolean name="enabled" value="($optical_preview==false)"/>'
ONE_SENSOR = '<sensor type="virtual_plane" id="coverage"><boolean name="enabled" value="($optical_preview==false &amp;&amp; $masked_overview==false)"/>'


def one_sensor_radio_xml():
    """_radio_city_xml where -Dmasked_overview=true leaves the overview camera as the only sensor (etoile.xml enables the coverage sensor
    beside it; one scene handle renders one film)."""
    x = _radio_city_xml()
    assert x.count(COVERAGE_ON) == 1
    return x.replace(COVERAGE_ON, ONE_SENSOR)


def masked_radio_xml(mask=MASK, sensor="perspective"):
    """one_sensor_radio_xml with `mask` in its perspective (or virtual-plane) sensor, as scenes/sionna_etoile/etoile.xml:77-79 has it."""
    x = one_sensor_radio_xml()
    if sensor == "perspective":
        tail = '<response type="RGB"/></film></sensor>'
    else:
        tail = '<response type="monochromatic"><spectrum type="discrete" wavelength="$wavelength"/></response></film></sensor>'
    assert x.count(tail) == 1
    return x.replace(tail, tail[:-len("</sensor>")] + mask + "</sensor>")


def _write(tmp_path, name, text):
    f = tmp_path / name
    f.write_text(text)
    return str(f)


def test_radio_scene_reads_the_mask(built, tmp_path):
    """The radio vocabulary with the etoile overview's mask: regex ^mesh-Plane$ (the `\\$` escape), 32 samples, exactly the ground plane
    flagged, and the same flattened scene, byte for byte, as the file without the mask."""
    from wave_tracer_amd import Scene
    d = {"masked_overview": "true"}
    a = Scene.from_xml(_write(tmp_path, "masked.xml", masked_radio_xml()), defines=d, res=64)
    b = Scene.from_xml(_write(tmp_path, "plain.xml", one_sensor_radio_xml()), defines=d, res=64)
    assert a.info.sensor_type == 0 and a.first_difference(b) == ""
    spec = a.sensor_mask_spec
    assert spec["regex"] == "^mesh-Plane$" and spec["samples"] == 32
    ids = a.shape_ids
    assert len(ids) == a.info.n_shapes == len(spec["shapes"]) and ids.count("mesh-Plane") == 1
    assert [ids[i] for i in np.flatnonzero(spec["shapes"])] == ["mesh-Plane"]
    assert all(i.startswith("__unnamed_$") for i in ids if i != "mesh-Plane")
    assert b.sensor_mask_spec is None and b.shape_ids == ids
    # from above: the ground plane is 0, roofs are 1, walls seen at an angle in between; every value is a multiple of 1/32
    m = a.sensor_mask_host()
    assert m.shape == (48, 64) and m.dtype == np.float32
    assert (m == 0).any() and (m == 1).any() and np.array_equal(m * 32, np.round(m * 32))
    assert np.array_equal(a.sensor_mask_host(seed=1), m) and np.array_equal(a.sensor_mask_host(threads=3), m)
    # the flags can come from the caller: all shapes "match" -> nothing is counted; none -> every hit counts
    assert not a.sensor_mask_host(shapes=np.ones(a.info.n_shapes)).any()
    assert (a.sensor_mask_host(shapes=np.zeros(a.info.n_shapes)) >= m).all()


# A camera 4 m above the ground looks straight down (60° field of view, square film): A is a ground rectangle that matches the regex, B abuts it
# at x = b1 and ends at x = b2, sky beyond.  Both extend far past the view along y, so every row of the mask is the same.
RES, H_CAM, FOV = 32, 4.0, 60.0
HW = H_CAM * math.tan(math.radians(FOV / 2))   # half width of the view on the ground
PW = 2 * HW / (RES - 1)                        # ground width of a pixel: the viewport spans width - 1 pixels (perspective.hpp:103-155)
B1, B2 = HW - 21.6 * PW, HW - 12.25 * PW       # inside pixel columns 21 and 12 (counted from +x)


def analytic_xml(regex=r"^A\$", extra_shape=""):
    return f'''<scene version="0.1.0">
  <integrator type="plt_path"><string name="direction" value="backward"/><integer name="max_depth" value="4"/></integrator>
  <sensor type="perspective"><quantity name="fov" value="{FOV}°"/>
    <transform name="to_world"><lookat origin="0m, 0m, {H_CAM}m" target="0m, 0m, 0m" up="0, 1, 0"/></transform>
    <film type="array"><integer name="width" value="{RES}"/><integer name="height" value="{RES}"/><response type="RGB"/></film>
    <sensor_mask type="by-geometry"><string name="mask_id_regex" value="{regex}"/></sensor_mask></sensor>
  <emitter type="directional"><transform name="to_world"><lookat target="0m,0m,0m" origin="1m,2m,5m" up="0,1,0"/></transform>
    <spectrum name="irradiance" blackbody="5500K"><float name="scale" value="5e-5"/></spectrum></emitter>
  <bsdf type="diffuse" id="grey"><spectrum rgb="0.5, 0.5, 0.5" name="reflectance"/></bsdf>
  <shape type="rectangle" id="A"><point name="p" x="-20m" y="-20m" z="0m"/><point name="x" x="{B1 + 20!r}m" y="0m" z="0m"/>
    <point name="y" x="0m" y="40m" z="0m"/><ref id="grey"/></shape>
  <shape type="rectangle" id="B"><point name="p" x="{B1!r}m" y="-20m" z="0m"/><point name="x" x="{B2 - B1!r}m" y="0m" z="0m"/>
    <point name="y" x="0m" y="40m" z="0m"/><ref id="grey"/></shape>
  {extra_shape}
</scene>'''


def _footprints(orientation):
    """Ground interval [x0, x1] of every pixel column, for the camera's x along +x (1) or -x (-1) of the world.  Film column c spans the camera
    x interval [HW - (c + 1) PW, HW - c PW] (the viewport mirrors x)."""
    c = np.arange(RES, dtype=np.float64)
    lo, hi = HW - (c + 1) * PW, HW - c * PW
    return (lo, hi) if orientation > 0 else (-hi, -lo)


def _share_over_b(orientation):
    x0, x1 = _footprints(orientation)
    return (np.clip(np.minimum(x1, B2) - np.maximum(x0, B1), 0, None)) / PW


def _seq_sum(n, samples):
    inc, v = np.float32(1) / np.float32(samples), np.float32(0)
    for _ in range(n):
        v = np.float32(v + inc)
    return v


def test_analytic_scene(built, tmp_path):
    """Pixels wholly over B are exactly 1, pixels over A or the sky exactly 0, the pixels on the two borders converge to their area share over B
    (mean over 24 seeds within 4 sigma of a binomial), and with 24 samples every value is the sequential f32 sum of n x (1/24.f)."""
    from wave_tracer_amd import Scene
    sc = Scene.from_xml(_write(tmp_path, "ab.xml", analytic_xml()))
    assert sc.shape_ids == ["A", "B"] and list(sc.sensor_mask_spec["shapes"]) == [1, 0]
    m = sc.sensor_mask_host(seed=3)
    # which way the film's x runs on the ground is read off the mask: one orientation must explain it
    fits = []
    for o in (1, -1):
        f = _share_over_b(o)
        full, none = f > 1 - 1e-9, f < 1e-9
        edge = ~(full | none)
        fits.append((o, full, none, edge, f))
    ok = [t for t in fits if (m[:, t[1]] == 1).all() and (m[:, t[2]] == 0).all()]
    assert len(ok) == 1
    _, full, none, edge, f = ok[0]
    assert full.sum() >= 8 and none.sum() >= 8 and edge.sum() == 2
    seeds = 24
    mean = np.mean([sc.sensor_mask_host(seed=s)[:, edge] for s in range(100, 100 + seeds)], axis=0).mean(axis=0)
    n = 32 * seeds * RES                                       # rows are alike: every row of the column is one more set of samples
    sigma = np.sqrt(f[edge] * (1 - f[edge]) / n)
    assert (np.abs(mean - f[edge]) < 4 * sigma).all(), (mean, f[edge], sigma)
    m24 = sc.sensor_mask_host(samples=24, seed=5)
    allowed = {float(_seq_sum(k, 24)): k for k in range(25)}
    assert all(float(v) in allowed for v in np.unique(m24))
    assert len(np.unique(m24[:, edge])) > 2 and (m24[:, full] == _seq_sum(24, 24)).all() and (m24[:, none] == 0).all()
    # seven samples per pixel: 1/7 does not add up to 1 exactly, the fully covered pixels hold the f32 sum of seven sevenths
    assert (sc.sensor_mask_host(samples=7)[:, full] == _seq_sum(7, 7)).all()
    # one sample per pixel: 0 or 1, nothing between; sixty-four: 1/64 adds up exactly, so every value is n/64 and the full pixels are 1
    m1 = sc.sensor_mask_host(samples=1, seed=5)
    assert np.isin(m1, [0, 1]).all() and (m1[:, full] == 1).all() and (m1[:, none] == 0).all() and len(np.unique(m1[:, edge])) == 2
    m64 = sc.sensor_mask_host(samples=64, seed=5)
    assert np.isin(m64, np.arange(65, dtype=np.float32) / np.float32(64)).all() and (m64[:, full] == 1).all() and (m64[:, none] == 0).all()
    assert len(np.unique(m64[:, edge])) > 2


def test_unnamed_shapes_are_numbered_like_the_reference(built, tmp_path):
    """Unnamed enabled top-level elements are __unnamed_$<n> (integrator 1, sensor 2, emitter 3, ..., loader.cpp:131-133); a regex can select one."""
    from wave_tracer_amd import Scene
    c = '''<shape type="rectangle"><point name="p" x="50m" y="50m" z="0m"/><point name="x" x="1m" y="0m" z="0m"/>
    <point name="y" x="0m" y="1m" z="0m"/><ref id="grey"/></shape>'''
    sc = Scene.from_xml(_write(tmp_path, "c.xml", analytic_xml(regex=r"^__unnamed_\\$4\$", extra_shape=c)))
    assert sc.shape_ids == ["A", "B", "__unnamed_$4"]
    spec = sc.sensor_mask_spec
    assert spec["regex"] == r"^__unnamed_\$4$" and list(spec["shapes"]) == [0, 0, 1]
    m = sc.sensor_mask_host()
    # A and B both count now: every column short of the sky edge is 1, every column beyond it 0
    fits = [(x1 <= B2, x0 >= B2) for x0, x1 in (_footprints(1), _footprints(-1))]
    assert any((m[:, ground] == 1).all() and (m[:, sky] == 0).all() and ground.sum() >= 12 and sky.sum() >= 8 for ground, sky in fits)


def test_mask_errors_and_quirks(built, tmp_path):
    from wave_tracer_amd import Scene, WtgpuError
    d = {"masked_overview": "true"}

    def load(mask, sensor="perspective", defines=d):
        return Scene.from_xml(_write(tmp_path, "m.xml", masked_radio_xml(mask, sensor)), defines=defines, res=32)
    with pytest.raises(WtgpuError, match=r"\(sensor mask loader\) Unrecognized 'type'"):
        load('<sensor_mask type="by-material"><string name="mask_id_regex" value="x"/></sensor_mask>')
    with pytest.raises(WtgpuError, match=r"expected 'mask_id_regex' regex expression to be provided"):
        load('<sensor_mask type="by-geometry"/>')
    with pytest.raises(WtgpuError, match=r"expected 'mask_id_regex'"):
        load('<sensor_mask type="by-geometry"><string name="mask_id_regex" value=""/></sensor_mask>')
    with pytest.raises(WtgpuError, match=r"invalid 'mask_id_regex'"):
        load('<sensor_mask type="by-geometry"><string name="mask_id_regex" value="mesh-([a-z"/></sensor_mask>')
    # the loader reads `samples` and never hands it to the mask (mask.cpp:93,105-107): still 32
    sc = load('<sensor_mask type="by-geometry"><integer name="samples" value="8"/><string name="mask_id_regex" value="^mesh-Plane\\$"/></sensor_mask>')
    assert sc.sensor_mask_spec["samples"] == 32
    assert np.array_equal(sc.sensor_mask_host(), sc.sensor_mask_host(samples=32)) and not np.array_equal(sc.sensor_mask_host(), sc.sensor_mask_host(samples=8))
    # a virtual-plane sensor reads no mask: ignored (with a warning), the same scene as without it; masks of such sensors are refused
    vp = load(MASK, "virtual_plane", defines={})
    assert vp.info.sensor_type == 1 and vp.sensor_mask_spec is None
    assert vp.first_difference(Scene.from_xml(_write(tmp_path, "p.xml", one_sensor_radio_xml()), res=32)) == ""
    with pytest.raises(WtgpuError, match="perspective sensor"):
        vp.sensor_mask_host(shapes=np.zeros(vp.info.n_shapes))
    # a scene without a mask needs the caller's flags; flags must cover every shape; bundled scenes have unnamed shapes
    from wave_tracer_amd import Scene as S
    box = S("cornell_box", res=16, mesh_detail=0)
    assert box.sensor_mask_spec is None and set(box.shape_ids) == {""}
    with pytest.raises(WtgpuError, match="no <sensor_mask>"):
        box.sensor_mask_host()
    with pytest.raises(ValueError):
        box.sensor_mask_host(shapes=[0])
    with pytest.raises(WtgpuError, match="samples"):
        box.sensor_mask_host(samples=0, shapes=np.zeros(box.info.n_shapes))
    m = box.sensor_mask_host(shapes=np.zeros(box.info.n_shapes))
    assert m.shape == (16, 16) and (m == 1).mean() > .5


def test_masked_writer_round_trips(tmp_path):
    """`<sensor>_tonemapped_masked.exr` (src/main.cpp:315-326): LA for a 1-component film, RGBA for a colour film, the mask as alpha."""
    from wave_tracer_amd.imageio import read_exr, write_masked
    rng = np.random.default_rng(4)
    mask = rng.uniform(0, 1, (6, 8)).astype(np.float32)
    mono = rng.uniform(0, 1, (6, 8, 1)).astype(np.float32)
    p = write_masked(str(tmp_path), "camera_perspective", "etoile", mono, mask, 1024)
    assert os.path.basename(p) == "camera_perspective_tonemapped_masked.exr"
    img, names, attrs = read_exr(p)
    assert sorted(names) == ["A", "Y"] and attrs["sensor"] == "camera_perspective_tonemapped" and attrs["samples"] == "1024"
    assert np.array_equal(img[..., names.index("Y")], mono[..., 0]) and np.array_equal(img[..., names.index("A")], mask)
    rgb = rng.uniform(0, 1, (6, 8, 3)).astype(np.float32)
    img, names, _ = read_exr(write_masked(str(tmp_path), "cam", "box", rgb, mask, 4))
    assert sorted(names) == ["A", "B", "G", "R"]
    assert all(np.array_equal(img[..., names.index(c)], rgb[..., i]) for i, c in enumerate("RGB")) and np.array_equal(img[..., names.index("A")], mask)
    with pytest.raises(ValueError):
        write_masked(str(tmp_path), "cam", "box", rgb, mask[:5], 4)


@pytest.mark.skipif(not os.path.exists(REF_ETOILE), reason="the reference checkout is not present on this machine")
def test_reference_etoile_reads_its_mask(built, tmp_path):
    """scenes/sionna_etoile/etoile.xml with -Dmasked_overview=true: the overview camera's mask.  The file enables the coverage sensor beside the
    camera; a copy with the coverage sensor switched off (meshes and data linked from the checkout) leaves the camera as the one film.  The
    copy also keeps the D65 point lamp that -Dmasked_overview=true disables: the two suns aim at the world's bounding box, which is empty when
    the checkout's meshes are Git-LFS pointers (skipped), and a scene without any emitter power is refused."""
    from wave_tracer_amd import Scene
    text = open(REF_ETOILE).read()
    a = text.index('<sensor type="virtual_plane" id="coverage">')
    b = text.index("</sensor>", a)
    on = 'value="($optical_preview==false)"'
    assert on in text[a:b]
    lamp = '<boolean name="enabled" value="($masked_overview==false)" />'
    assert text.count(lamp) == 1 and text.index(lamp) > b
    text = text[:a] + text[a:b].replace(on, 'value="false"', 1) + text[b:].replace(lamp, "")
    (tmp_path / "meshes").symlink_to(os.path.join(os.path.dirname(REF_ETOILE), "meshes"))
    (tmp_path / "data").symlink_to(os.path.join(os.path.dirname(REF_ETOILE), "..", "..", "data"))
    sc = Scene.from_xml(_write(tmp_path, "etoile.xml", text), defines={"masked_overview": "true", "wtgpu_missing_assets": "skip"}, res=64)
    spec = sc.sensor_mask_spec
    assert sc.info.sensor_type == 0 and spec["regex"] == "^mesh-Plane$" and spec["samples"] == 32 and len(spec["shapes"]) == sc.info.n_shapes
    assert {sc.shape_ids[i] for i in range(sc.info.n_shapes) if spec["shapes"][i]} <= {"mesh-Plane"}
