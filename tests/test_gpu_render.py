"""GPU parity tests proper: the HIP path (through the C-ABI) against the CPU checker on identical seeded inputs."""
import numpy as np
import pytest

from oracle_util import oracle_render
import parity

pytestmark = pytest.mark.gpu


def _both(name, res, spp, seed, **kw):
    from wave_tracer_amd import Scene, render, develop
    sc = Scene(name, res=res, **kw)
    v, w, l = render(sc, spp, seed=seed, device=0)
    gpu = develop(sc, v, w, l, spp).astype(np.float64)
    gc = sc.counters()
    ov, ow, ol, oc = oracle_render(sc, 0, spp, seed)
    cpu = develop(sc, ov, ow, ol, spp).astype(np.float64)
    return sc, gpu, cpu, gc, oc, (v, w, l), (ov, ow, ol)


def _rel_l1(a, b):
    return np.abs(a - b).sum() / max(1e-300, np.abs(b).sum())


@pytest.mark.parametrize("name,res,spp,kw", [
    ("furnace", 32, 4, {}),
    ("white_furnace", 24, 8, {}),
    ("furnace", 24, 4, {"fsd": 1, "lut": (128, 128)}),
    # rough conductors with the Gaussian (roughness-parametrised and explicit rms) and the fractal surface profile
    ("furnace_spm", 32, 8, {}),
    # double_slits.xml -Doptical_overview=true: ray-trace-only RGB camera, two directional emitters, RGB-uplifted reflectances
    ("double_slits_overview", 32, 8, {"lut": (64, 64)}),
    # dispatching BSDF wrappers evaluated per sample on the device: composite bins on both sides of the 550 nm boundary, a bin gap
    # (no BSDF), a stochastic mask with its null lobe (tests/test_wrappers.py has the semantics)
    ("furnace_wall_composite", 24, 8, {}),
    ("furnace_wall_composite_gap", 24, 8, {}),
    ("furnace_wall_mask", 24, 8, {}),
    # textures on the device: checkerboard reflectance under a uv transform, a bilinear bitmap, a textured mask, a normal map
    # (tests/test_textures.py has the semantics)
    ("tex_checker", 32, 8, {}),
    ("tex_bilinear_ramp", 32, 8, {}),
    ("tex_mask", 32, 8, {}),
    ("tex_normal_tilt", 32, 8, {}),
    # subpaths of up to 34 / 42 vertices (max_depth beyond the 16 of rounds 1-2; Russian roulette off so that the walks really get there):
    # vertex stores sized from the scene, streaming MIS weights, the open-ended last row / column of the strategy buckets
    ("furnace", 16, 4, {"max_depth": 32, "rr": 0}),
    ("white_furnace", 12, 4, {"max_depth": 40, "rr": 0}),
])
def test_image_parity_small(built, name, res, spp, kw):
    """Same Philox streams on both sides => the images agree sample for sample up to fp contraction / libm ulps.
    Tolerance: relative L1 error of the developed image < 1e-2 (a handful of samples take a different discrete branch)."""
    sc, gpu, cpu, gc, oc, gf, cf = _both(name, res, spp, 5, **kw)
    assert np.isfinite(gpu).all()
    # film weights are pure geometry: must agree to fp32 rounding
    assert np.allclose(gf[1], cf[1], rtol=1e-5, atol=1e-6)
    parity.check(f"image_parity_small/{name}-{res}-{spp}-{sorted(kw.items())}", _rel_l1(gpu, cpu), 1e-2)
    for key in ("segments", "vertices", "connections", "surface_interactions"):
        assert abs(gc[key] - oc[key]) <= 2e-3 * max(1, oc[key]), (key, gc[key], oc[key])


@pytest.mark.parametrize("name,res,spp,kw,tol", [
    # wave-optics case: ~15 % of the vertices are free-space-diffraction interactions (rejection sampling, LUT inversion)
    ("double_slits", 96, 8, {"lut": (128, 128)}, 2e-2),
    # the headline scene (small film, coarse stand-in meshes): all BSDFs, spectra, both emitter types, dielectrics
    # (central crop of the 1440^2 film: same pixel pitch and hence the same beam footprints as the headline workload)
    ("cornell_box", 32, 4, {"mesh_detail": 0, "lut": (128, 128), "crop_of": 1440}, 2e-2),
])
def test_image_parity_scenes(built, name, res, spp, kw, tol):
    sc, gpu, cpu, gc, oc, gf, cf = _both(name, res, spp, 7, **kw)
    assert np.isfinite(gpu).all()
    assert np.allclose(gf[1], cf[1], rtol=1e-5, atol=1e-6)
    parity.check(f"image_parity_scenes/{name}-{res}-{spp}-{sorted(kw.items())}", _rel_l1(gpu, cpu), tol)
    for key in ("segments", "vertices", "connections", "surface_interactions"):
        assert abs(gc[key] - oc[key]) <= 5e-3 * max(20, oc[key]), (key, gc[key], oc[key])
    # the bounded device triangle list can change which silhouette edges a wide beam sees: 2 %
    assert abs(gc["fsd_interactions"] - oc["fsd_interactions"]) <= 2e-2 * max(50, oc["fsd_interactions"])
    assert gc["walk_iteration_cap_hits"] == 0


def test_cornell_dense_mesh_parity(built):
    """Bench geometry (283K triangles: bounded lists, cooperative heavy-walk kernel, whole-region edge / power gathers all active) on
    a small film.  Interaction regions are unbounded on both sides now (the device walks regions that overflow its 64-triangle list
    once more: resolve_primary, k_edges, k_flux_*), so what remains are traversal-order details: the reference's (and the CPU
    checker's) list of a region also holds triangles it met before the region's slab shrank, the device's gathers use the final slab.
    Tolerance 2 % relative L1 on the image, 0.5 % on event counts, 1.5 % on the number of diffraction interactions."""
    sc, gpu, cpu, gc, oc, gf, cf = _both("cornell_box", 64, 4, 3, mesh_detail=1, lut=(128, 128), crop_of=1440)
    assert np.isfinite(gpu).all()
    assert np.allclose(gf[1], cf[1], rtol=1e-5, atol=1e-6)
    print("dense crop: rel L1", _rel_l1(gpu, cpu), "fsd", gc["fsd_interactions"], oc["fsd_interactions"], "overflow counters",
          {k: gc[k] for k in ("edge_overflow", "fsd_edge_overflow", "fsd_pool_overflow")}, {k: oc[k] for k in ("edge_overflow", "fsd_edge_overflow")})
    parity.check("cornell_dense_mesh_parity", _rel_l1(gpu, cpu), 2e-2)
    for key in ("segments", "vertices", "connections"):
        assert abs(gc[key] - oc[key]) <= 5e-3 * oc[key], (key, gc[key], oc[key])
    assert abs(gc["fsd_interactions"] - oc["fsd_interactions"]) <= 1.5e-2 * oc["fsd_interactions"] + 3, (gc["fsd_interactions"], oc["fsd_interactions"])
    assert gc["fsd_pool_overflow"] == 0


@pytest.mark.parametrize("case", ["furnace_r16", "furnace_fsd_r16", "white_furnace_r12", "double_slits_r96", "cornell_box_r12", "etoile_r48",
                                  "white_furnace_path_r12", "sunlit_r16", "cornell_box_stokes_r12"])
def test_gpu_matches_committed_golden(built, case):
    """tests/golden/*.npz are THIS repository's checker output (tests/golden/make_golden.py), committed: they pin regressions of the device path
    and of the checker against a fixed state of both, not correctness against the reference (no reference output exists here; what pins the
    checker is in DESIGN.md §7: closed forms, the second composition, second-source primitives)."""
    import json
    import os
    from golden.make_golden import CASES, run_case
    from wave_tracer_amd import render

    def gpu_renderer(sc, b, e, seed):
        v, w, l = render(sc, e - b, seed=seed, device=0, sample_begin=b)
        return v, w, l, sc.counters()

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", case + ".npz"))
    meta = json.loads(str(g["meta"]))
    img, counters = run_case(CASES[case], renderer=gpu_renderer)
    ref = g["image"].astype(np.float64)
    parity.check(f"committed_golden/{case}", np.abs(img - ref).sum() / np.abs(ref).sum(), 2e-2)
    for k, v in meta["counters"].items():
        tol = 3e-2 if k == "fsd_interactions" else 5e-3      # bounded device triangle lists: see test_image_parity_scenes
        assert abs(counters[k] - v) <= tol * max(50, v), (k, counters[k], v)


def test_sample_range_additivity_and_determinism(built):
    """Films are linear accumulators: rendering [0,4) equals [0,2) + [2,4); the same range twice gives the same film up to
    the order of the f64 atomic adds."""
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace", res=32, lut=(32, 32))
    v, w, l = render(sc, 4, seed=9)
    va, wa, la = render(sc, 2, seed=9, sample_begin=0)
    vb, wb, lb = render(sc, 2, seed=9, sample_begin=2)
    assert np.allclose(va + vb, v, rtol=1e-9, atol=1e-30) and np.allclose(wa + wb, w, rtol=1e-12) and np.allclose(la + lb, l, rtol=1e-9, atol=1e-30)
    v2, w2, l2 = render(sc, 4, seed=9)
    assert np.allclose(v2, v, rtol=1e-9, atol=1e-30) and np.array_equal(w2 > 0, w > 0)
    v3, _, _ = render(sc, 4, seed=10)
    assert not np.allclose(v3, v)


def test_batched_render_equals_unbatched(built):
    """max_batch_samples smaller than the film: the render is split into launches over pixel ranges; same result."""
    from wave_tracer_amd import Scene, render
    a = Scene("furnace", res=32, lut=(32, 32))
    a.upload(0, 0)
    b = Scene("furnace", res=32, lut=(32, 32))
    b.upload(0, 300)            # ragged: 1024 pixels in batches of 300
    va, wa, la = render(a, 2, seed=4)
    vb, wb, lb = render(b, 2, seed=4)
    assert b.timings()["batches"] >= 4
    assert np.allclose(va, vb, rtol=1e-9, atol=1e-30) and np.allclose(wa, wb, rtol=1e-12) and np.allclose(la, lb, rtol=1e-9, atol=1e-30)


def test_scene_from_desc_renders_like_the_named_scene(built):
    """wtgpu_scene_create_from_desc + upload + render == the named scene it was taken from."""
    from wave_tracer_amd import Scene, render
    a = Scene("furnace", res=24, lut=(32, 32))
    b = Scene.from_desc(a.host_desc(), keepalive=a)
    va, wa, la = render(a, 4, seed=6)
    vb, wb, lb = render(b, 4, seed=6)
    assert np.allclose(wa, wb, rtol=1e-12) and np.abs(va - vb).sum() <= 1e-9 * np.abs(va).sum() and np.abs(la - lb).sum() <= 1e-9 * max(np.abs(la).sum(), 1e-300)
    assert a.counters() == b.counters()


def test_async_renders_pipeline_and_join(built):
    """wtgpu_render_async + wtgpu_join: several un-joined renders into the same accumulators equal one joined render."""
    import torch
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import alloc_films
    sc = Scene("furnace", res=32, lut=(32, 32))
    ref = render(sc, 6, seed=21)
    dev = torch.device("cuda", 0)
    v, w, l = alloc_films(sc, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for s in range(6):
        sc.render_async_into(v, w, l, s, s + 1, 21, st)
    sc.join(st)
    torch.cuda.synchronize(dev)
    for a, b in zip((v, w, l), ref):
        assert np.allclose(a.cpu().numpy(), b, rtol=1e-9, atol=1e-30)


def test_tiled_film_splat_equals_the_per_sample_splat(built, monkeypatch):
    """k_connect_splat_tiled (one block per 64-element row segment, footprints accumulated in an LDS tile, one global add per tile entry) against
    the per-sample splat kernel (WTGPU_TILED_SPLAT=0): the same films up to the order of the f64 sums — intensity and Stokes films, widths that
    are not multiples of the block, several samples per element and batch, batches that start in the middle of the film."""
    import torch
    from wave_tracer_amd import Scene, render
    for name, kw, batch in (("cornell_box", dict(res=150, mesh_detail=0), 0), ("bidir_room", dict(res=136, mesh_detail=0, polarimetric=1), 0),
                            ("furnace", dict(res=40, lut=(32, 32)), 1000)):
        out = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("WTGPU_TILED_SPLAT", mode)
            sc = Scene(name, **kw)
            sc.upload(0, batch if batch else 3 * sc.width * sc.height)
            out[mode] = render(sc, 5, seed=31)
            sc.close()
        assert out["0"][0].sum() > 0 and out["0"][1].sum() > 0
        for a, b in zip(out["0"], out["1"]):
            assert np.allclose(a, b, rtol=1e-9, atol=1e-30), name


def test_two_renders_of_one_batch_give_the_same_value_film(built):
    """k_connect_splat_tiled adds the tiles that meet in a film element in a FIXED order: one wavefront per 64-element row segment, its blocks in six
    launches by (row % 3, segment % 2) (wtgpu_kernels.h: kSplatPhases).  So two renders of the same single batch give the same value and weight films bit
    for bit — before, the last bit of a few elements depended on which block came first.  Shapes: 1, 2, 3 and 4 segments per row (odd and even), heights
    0, 1 and 2 mod 3, intensity and Stokes films, two samples per element.  (The light image is not this kernel's: it is splatted by the connections.)"""
    from wave_tracer_amd import Scene, render
    shapes = set()
    for name, kw in (("furnace", dict(res=40, lut=(32, 32))), ("cornell_box", dict(res=100, mesh_detail=0)), ("cornell_box", dict(res=150, mesh_detail=0)),
                     ("cornell_box", dict(res=200, mesh_detail=0)), ("bidir_room", dict(res=136, mesh_detail=0, polarimetric=1))):
        sc = Scene(name, **kw)
        sc.upload(0, 2 * sc.width * sc.height)
        shapes.add(((sc.width + 63) // 64, sc.height % 3))
        a, b = [render(sc, 2, seed=41) for _ in range(2)]
        sc.close()
        assert np.asarray(a[0]).sum() > 0 and np.asarray(a[1]).sum() > 0
        for x, y, film in zip(a[:2], b[:2], ("value", "weight")):
            x, y = np.asarray(x), np.asarray(y)
            assert np.array_equal(x, y), (name, kw["res"], film, int((x != y).sum()))
    assert {s for s, _ in shapes} >= {1, 2, 3, 4} and {h for _, h in shapes} == {0, 1, 2}, shapes


def test_batches_enqueued_in_two_parts_render_the_same(built, monkeypatch):
    """A batch is enqueued in two parts (wtgpu.hip: batch_launcher_t): the rounds its walks are expected to need, and — once the host has seen
    the round queue empty, or has launched ALL the remaining rounds — the connections.  Whatever the expectation, the film is the one a blind
    launch of every round gives: WTGPU_FIRST_ROUNDS=96 (every round up front, as before round 4), =2 (every batch needs several more
    looks), and the default (adaptive: after the first batches only the rounds that have work, + a margin, are launched).  Many small
    batches, both integrators."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    for name, kw in (("cornell_box", dict(res=48, mesh_detail=0)), ("etoile", dict(res=48, mesh_detail=0))):
        out = {}
        for mode in ("96", "2", "0", "2-nolight"):
            # ("2": from the third round on the batch's walks run as LIGHT ROUNDS — k_light_rounds: trace, pass A and pass B of every round in one
            # one-block launch that stops before any stage it does not hold — "2-nolight": the same rounds as ordinary rounds, eight at a time)
            monkeypatch.setenv("WTGPU_FIRST_ROUNDS", mode.split("-")[0])
            monkeypatch.setenv("WTGPU_LIGHT_ROUNDS", "0" if mode.endswith("nolight") else "1")
            sc = Scene(name, **kw)
            sc.upload(0, 512)                       # 512 samples per batch: ~4 batches per sample per element
            dev = torch.device("cuda", 0)
            films = alloc_films(sc, dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            sc.reset_counters()
            for i in range(6):
                sc.render_async_into(*films, i, i + 1, 77, st)
            sc.join(st)
            torch.cuda.synchronize(dev)
            c, t = sc.counters(), sc.timings()
            out[mode] = ([f.cpu().numpy() for f in films], c, t)
            sc.close()
        ref, cref, tref = out["96"]
        assert tref["rounds_per_batch"] == 96
        for mode in ("2", "0", "2-nolight"):
            films, c, t = out[mode]
            for a, b in zip(films, ref):
                assert np.allclose(a, b, rtol=1e-9, atol=1e-30), (name, mode)
            for k in ("samples", "segments", "vertices", "connections", "fsd_interactions", "light_splats", "walk_iteration_cap_hits"):
                assert c[k] == cref[k], (name, mode, k, c[k], cref[k])
        with_work = tref["rounds"] / tref["batches"]
        assert with_work <= out["2"][2]["rounds_per_batch"] <= with_work + 10      # every batch: 2 rounds, then 8 at a time until the queue is empty
        print(name, "rounds launched per batch, adaptive:", out["0"][2]["rounds_per_batch"], "with work:", tref["rounds"] / tref["batches"])
        assert out["0"][2]["rounds_per_batch"] <= with_work + 16   # (the first batches guess 32; afterwards: the recent mean + 2, then 8 at a time)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,spp", [("cornell_box", dict(res=48, mesh_detail=0), 4), ("bidir_room", dict(res=48), 2), ("furnace_wall_mask", dict(res=24), 8),
                                         ("furnace_spm", dict(res=32), 4), ("double_slits", dict(res=96, lut=(64, 64)), 2)])
def test_material_sorted_pass_and_staged_connections_render_the_same(built, monkeypatch, name, kw, spp):
    """The interaction pass sorted by material class (k_classify + one kernel per BSDF class, or the one-launch form with work stealing) and the
    connections in three stages (k_connect_eval -> k_connect_shadow -> k_connect_mis, in chunks that cannot overflow their pending list) against
    the one-kernel forms: the same walks, vertices and connections (every counter equal), the same films up to the order of the f64 / f32 sums."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    out = {}
    for mode in ((0, 0), (1, 0), (2, 0), (0, 1), (2, 1)):
        monkeypatch.setenv("WTGPU_SORTED_INTERACT", str(mode[0]))
        monkeypatch.setenv("WTGPU_STAGED_CONNECT", str(mode[1]))
        monkeypatch.setenv("WTGPU_CONN_POOL", "2")   # (two pending records per sample: several chunks have work)
        sc = Scene(name, **kw)
        sc.upload(0, 2048)
        dev = torch.device("cuda", 0)
        films = alloc_films(sc, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        sc.reset_counters()
        sc.render_into(*films, 0, spp, 31, st)
        torch.cuda.synchronize(dev)
        out[mode] = ([f.cpu().numpy() for f in films], sc.counters())
        sc.close()
    ref, cref = out[(0, 0)]
    assert cref["surface_interactions"] > 1000 and cref["connections"] > 1000 and cref["shadow_rays"] > 100
    for mode, (films, c) in out.items():
        assert c == cref, (mode, c, cref)
        for a, b in zip(films, ref):
            assert np.allclose(a, b, rtol=2e-6, atol=1e-12 * max(1.0, float(np.abs(b).max()))), (name, mode, float(np.abs(a - b).max()))


def test_empty_sample_range_is_a_noop(built):
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace", res=16, lut=(32, 32))
    v, w, l = render(sc, 0, seed=1)
    assert not v.any() and not w.any() and not l.any()


def test_full_size_properties_1440(built):
    """BASELINE.json's full size (cornell box 1440x1440, 2,073,600 samples per pass), too big for the CPU checker:
    size-independent properties.  (1) every film value finite and non-negative; (2) the weight film is pure geometry: one
    pass deposits exactly one unit of reconstruction weight per sample, minus what falls off the border; (3) film linearity
    at full size: two 1-spp passes sum to the 2-spp pass; (4) event statistics per sample agree with a 96x96 CPU-checker
    render of the same scene within 3 % (they are resolution independent)."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    sc = Scene("cornell_box", res=1440, mesh_detail=1)
    sc.upload(0, 1440 * 1440)
    dev = torch.device("cuda", 0)
    films = [alloc_films(sc, dev) for _ in range(3)]
    st = torch.cuda.current_stream(dev).cuda_stream
    sc.reset_counters()
    sc.render_into(*films[0], 0, 1, 5, st)
    sc.render_into(*films[1], 1, 2, 5, st)
    c = sc.counters()
    sc.render_into(*films[2], 0, 2, 5, st)
    torch.cuda.synchronize(dev)
    for v, w, l in films:
        assert torch.isfinite(v).all() and torch.isfinite(w).all() and torch.isfinite(l).all()
        assert (v >= 0).all() and (w >= 0).all() and (l >= 0).all()
    npix = 1440 * 1440
    wsum = float(films[0][1].sum())
    assert 0.995 * npix < wsum <= npix * (1 + 1e-6), wsum / npix
    for k in range(3):
        s = films[0][k] + films[1][k]
        assert torch.allclose(s, films[2][k], rtol=1e-7, atol=1e-30)
    assert c["samples"] == 2 * npix and c["walk_iteration_cap_hits"] == 0
    # (5) sample-for-sample parity AT FULL SIZE on a bounded sample of the workload: the CPU checker renders every 97th 24x24
    # block of the same 1440^2 film (38 blocks, 21,888 samples).  Pixels >= 1 px inside those blocks receive `value`/`weight`
    # splats only from samples of their own block (3x3 reconstruction filter), so they are directly comparable; `light`
    # (t<=1 splats from anywhere on the film) is not.  Tolerance: the bounded device lists make a few samples
    # differ: relative L1 over the compared pixels < 5 %, weights to fp32 rounding.
    from oracle_util import oracle_render_tiles
    ov, ow, ol, oc5, n5, mask = oracle_render_tiles(sc, 0, 1, 5, 97)
    inner = mask.copy()
    inner[1:, :] &= mask[:-1, :]
    inner[:-1, :] &= mask[1:, :]
    inner[:, 1:] &= mask[:, :-1]
    inner[:, :-1] &= mask[:, 1:]
    inner[0, :] = inner[-1, :] = inner[:, 0] = inner[:, -1] = False
    gv, gw = films[0][0].cpu().numpy(), films[0][1].cpu().numpy()
    assert inner.sum() > 15000
    assert np.allclose(gw[inner], ow[inner], rtol=1e-5, atol=1e-7)
    rel = np.abs(gv[inner] - ov[inner]).sum() / np.abs(ov[inner]).sum()
    frac_same = (np.abs(gv[inner] - ov[inner]).sum(axis=1) <= 1e-3 * np.abs(ov[inner]).sum(axis=1) + 1e-30).mean()
    print("full size: rel L1", rel, "frac_same", frac_same, "counters", {k: c[k] for k in ("edge_overflow", "fsd_edge_overflow", "fsd_pool_overflow", "fsd_interactions")},
          "oracle tiles", {k: oc5[k] for k in ("edge_overflow", "fsd_edge_overflow", "fsd_interactions")})
    parity.check("full_size_properties_1440/blocks_value", rel, 2e-2)
    assert frac_same > 0.99, frac_same
    # (6) the WHOLE film — value, weight and the light plane (the t <= 1 splats, which land anywhere on the film and cannot be compared block by
    # block) — against the checker rendering all 2,073,600 samples of the same pass (15 s on the GPU box's host cores)
    fv, fw, fl, fc = oracle_render(sc, 0, 1, 5)
    g0 = [t.cpu().numpy() for t in films[0]]
    assert np.allclose(g0[1], fw, rtol=1e-5, atol=1e-7)
    parity.check("full_size_properties_1440/light_plane", np.abs(g0[2] - fl).sum() / np.abs(fl).sum(), 2e-2)
    parity.check("full_size_properties_1440/light_sum", abs(g0[2].sum() - fl.sum()) / fl.sum(), 2e-3)
    parity.check("full_size_properties_1440/value_plane", np.abs(g0[0] - fv).sum() / np.abs(fv).sum(), 2e-2)
    from wave_tracer_amd import develop
    gi, oi = develop(sc, *g0, 1).astype(np.float64), develop(sc, fv, fw, fl, 1).astype(np.float64)
    parity.check("full_size_properties_1440/developed_image", np.abs(gi - oi).sum() / np.abs(oi).sum(), 2e-2)
    print("full size, whole film: light rel L1", np.abs(g0[2] - fl).sum() / np.abs(fl).sum(), "light sums", g0[2].sum(), fl.sum(), "image rel L1", np.abs(gi - oi).sum() / np.abs(oi).sum())
    # 5 % of the diffusive segments of this workload see more than kMaxConeTris = 64 triangles (CPU profile: p99 = 2400, max
    # 82,000): those regions are walked in full on the device, so all but a fraction of a per cent of the pixels agree
    # with the CPU checker's unbounded lists to fp32 rounding
    assert frac_same > 0.99, frac_same
    # nothing was capped or dropped on the HEADLINE workload: per-lane edge sets, aperture segments, the aperture pool, the cooperative stack
    for key in ("fsd_pool_overflow", "edge_overflow", "fsd_edge_overflow", "traversal_stack_dropped"):
        assert c[key] == 0, (key, c[key])
    small = Scene("cornell_box", res=96, mesh_detail=1)
    _, _, _, oc = oracle_render(small, 0, 2, 5)
    n_small = 96 * 96 * 2
    # sanity only: the 96^2 film has 15x wider pixel beams, hence more diffusive/diffractive events per sample
    for key in ("segments", "vertices", "connections"):
        a, b = c[key] / c["samples"], oc[key] / n_small
        assert abs(a - b) < 0.25 * b, (key, a, b)


def test_xml_scene_renders_like_the_checker(built):
    """A scene loaded by the minimal XML reader (tests/data/xml/single_slit.xml: spot + slit in a conducting screen + wall sensor) goes
    through the same C-ABI: GPU == CPU checker on the same random numbers."""
    import os
    from wave_tracer_amd import Scene, render, develop
    sc = Scene.from_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "xml", "single_slit.xml"), res=128, lut=(128, 128))
    spp = 8
    v, w, l = render(sc, spp, seed=21)
    ov, ow, ol, oc = oracle_render(sc, 0, spp, 21)
    gi, oi = develop(sc, v, w, l, spp).astype(np.float64), develop(sc, ov, ow, ol, spp).astype(np.float64)
    assert oc["fsd_interactions"] > 100 and oi.sum() > 0
    parity.check("xml_scene_renders_like_the_checker", np.abs(gi - oi).sum() / np.abs(oi).sum(), 2e-2)
    c = sc.counters()
    assert abs(c["fsd_interactions"] - oc["fsd_interactions"]) <= 0.02 * oc["fsd_interactions"]


@pytest.mark.parametrize("variant,fn", [(2, None), (3, None), (4, "0.5 + 0.3*sin(2*pi*3*u) * cos(2*pi*2*v) * (k > 11424)"), (7, None)])
def test_function_textures_render_like_the_checker(built, variant, fn):
    """Function / mix textures and a textured roughness (tests/data/xml/function_textures.xml: the device interprets the compiled expression,
    wt/scene.h texture_function) through the C-ABI: GPU == CPU checker on the same random numbers."""
    import os
    from wave_tracer_amd import Scene, render, develop
    defines = {"variant": variant}
    if fn:
        defines["fn"] = fn
    sc = Scene.from_xml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "xml", "function_textures.xml"), defines=defines, res=64)
    spp = 8
    v, w, l = render(sc, spp, seed=9)
    ov, ow, ol, oc = oracle_render(sc, 0, spp, 9)
    gi, oi = develop(sc, v, w, l, spp).astype(np.float64), develop(sc, ov, ow, ol, spp).astype(np.float64)
    assert oi.sum() > 0 and np.allclose(w, ow, rtol=1e-5, atol=1e-7)
    parity.check(f"function_textures/{variant}", _rel_l1(gi, oi), 1e-2)
    c = sc.counters()
    for key in ("segments", "vertices", "connections"):
        assert abs(c[key] - oc[key]) <= 5e-3 * oc[key], (key, c[key], oc[key])


def test_double_slits_full_size_1440(built):
    """BASELINE.json configs[0] at its real size (scenes/diffraction_simple/double_slits.xml with res = 1440: virtual-plane film
    1440 x 360, 518,400 samples per pass).  The scene is small enough for the CPU checker to render the whole film, so this is a
    FULL parity test at full size, plus the size-independent properties:
      (1) finite, non-negative; two 1-spp passes sum to the 2-spp pass (film linearity);
      (2) GPU == CPU checker on the same random numbers: weights to fp32 rounding, developed image rel-L1 < 2e-2, event counters
          within 0.5 %;
      (3) physics at 32 spp: the column profile outside the geometric shadow boundary follows cos^2(pi d x / lambda L) sinc^2(a x /
          lambda L) (correlation > 0.985), bright orders at +-4.6 / 14.7 / 24.8 mm, left-right symmetric within 5 %."""
    import torch
    from wave_tracer_amd import Scene, develop
    from wave_tracer_amd.render import alloc_films
    res = 1440
    sc = Scene("double_slits", res=res)
    assert (sc.width, sc.height) == (1440, 360)
    sc.upload(0)
    dev = torch.device("cuda", 0)
    films = [alloc_films(sc, dev) for _ in range(4)]
    st = torch.cuda.current_stream(dev).cuda_stream
    sc.reset_counters()
    sc.render_into(*films[0], 0, 1, 9, st)
    sc.render_into(*films[1], 1, 2, 9, st)
    torch.cuda.synchronize(dev)
    c = sc.counters()
    sc.render_into(*films[2], 0, 2, 9, st)
    sc.render_into(*films[3], 0, 32, 10, st)
    torch.cuda.synchronize(dev)
    for v, w, l in films:
        assert torch.isfinite(v).all() and torch.isfinite(w).all() and torch.isfinite(l).all()
        assert (v >= 0).all() and (w >= 0).all() and (l >= 0).all()
    for k in range(3):
        assert torch.allclose(films[0][k] + films[1][k], films[2][k], rtol=1e-7, atol=1e-30)
    assert c["samples"] == 2 * sc.width * sc.height and c["walk_iteration_cap_hits"] == 0 and c["traversal_stack_dropped"] == 0
    assert c["edge_overflow"] == 0 and c["fsd_edge_overflow"] == 0 and c["fsd_pool_overflow"] == 0
    # (2) full-film parity
    ov, ow, ol, oc = oracle_render(sc, 0, 2, 9)
    g = [t.cpu().numpy() for t in films[2]]
    assert np.allclose(g[1], ow, rtol=1e-5, atol=1e-7)
    gi, oi = develop(sc, *g, 2).astype(np.float64), develop(sc, ov, ow, ol, 2).astype(np.float64)
    rel = np.abs(gi - oi).sum() / np.abs(oi).sum()
    print("double slits 1440x360: rel L1", rel, {k: (c[k], oc[k]) for k in ("segments", "vertices", "fsd_interactions", "light_splats")})
    parity.check("double_slits_full_size_1440/image", rel, 2e-2)
    for k in ("segments", "vertices", "connections", "fsd_interactions", "light_splats"):
        assert abs(c[k] - oc[k]) <= 5e-3 * max(oc[k], 200), (k, c[k], oc[k])
    # (3) fringes
    img = develop(sc, *[t.cpu().numpy() for t in films[3]], 32).astype(np.float64)
    prof = img.sum(axis=(0, 2))
    x = (np.arange(res) + .5 - res / 2) * 250.0 / res                   # mm on the wall
    lamL, d, a = 3.25, .65, .35
    ana = np.cos(np.pi * d * x / lamL) ** 2 * np.sinc(a * x / lamL) ** 2
    m = (np.abs(x) > 2.8) & (np.abs(x) < 32)
    # (columns are 0.17 mm wide here: smooth the Monte-Carlo noise of single columns over 1 mm before comparing shapes)
    ker = np.ones(6) / 6
    ps, as_ = np.convolve(prof, ker, "same"), np.convolve(ana, ker, "same")
    assert np.corrcoef(ps[m] / ps[m].max(), as_[m] / as_[m].max())[0, 1] > 0.985
    assert abs(prof[x > 0].sum() / prof[x < 0].sum() - 1) < 0.05
    for lo, hi, centre in [(2.8, 8, 4.6), (12, 18, 14.7), (22, 28, 24.8)]:
        for sgn in (1, -1):
            w_ = (sgn * x > lo) & (sgn * x < hi)
            assert abs(abs(x[w_][np.argmax(ps[w_])]) - centre) < 0.8


def test_rmse_far_below_monte_carlo_noise_floor(built):
    """BASELINE.json's second metric is the image RMSE against the CPU reference.  With identical random numbers the GPU image
    differs from the CPU checker's by far less than two CPU renders with different seeds differ from each other (the Monte-Carlo
    noise floor at this sample count): normalised RMSE < 3e-2 and < 1/20 of the floor on the diffraction gate scene."""
    from wave_tracer_amd import Scene, render, develop
    sc = Scene("double_slits", res=360, lut=(256, 256))
    spp = 16
    v, w, l = render(sc, spp, seed=7)
    g = develop(sc, v, w, l, spp).astype(np.float64)
    ov, ow, ol, _ = oracle_render(sc, 0, spp, 7)
    c = develop(sc, ov, ow, ol, spp).astype(np.float64)
    ov2, ow2, ol2, _ = oracle_render(sc, 0, spp, 8)
    c2 = develop(sc, ov2, ow2, ol2, spp).astype(np.float64)

    def nrmse(a, b):
        return float(np.sqrt(np.mean((a - b) ** 2)) / np.mean(b))
    same, floor = nrmse(g, c), nrmse(c2, c)
    assert same < 3e-2 and same < floor / 20, (same, floor)


def test_c_host_smoke_program(built):
    """The plain-C host of the C-ABI (csrc/smoke.c): named scene + description round trip + progressive render + develop on the GPU."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output([os.path.join(root, "wave_tracer_amd", "wtgpu_smoke")]).decode()
    assert "smoke.c: furnace 24x24, 4 spp" in out and "4 progress calls" in out, out


def test_enqueue_is_not_throttled_by_the_runtime(built):
    """wtgpu_render_async returns when a pass is ENQUEUED.  The HIP runtime stages by-value kernel arguments in a ring per stream (1 MiB by
    default); a batch is ~870 launches of a ~1 KB launch block, and a full ring blocks the enqueueing thread until the GPU has caught up —
    which serialises the internal streams (976 -> 1048 bytes of arguments, or one more kernel per round, cost 40 % of a
    pass).  With HSA_KERNARG_POOL_SIZE raised by the package (before HIP initialises) the enqueue of a 720^2 pass takes a few ms; throttled
    it takes about as long as the pass itself.  Guards the launch block's size, the number of launches per batch and the runtime setting."""
    import os
    import time
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    assert int(os.environ.get("HSA_KERNARG_POOL_SIZE", "0")) >= (4 << 20)
    sc = Scene("cornell_box", res=720)
    sc.upload(0, sc.width * sc.height)
    dev = torch.device("cuda", 0)
    films = alloc_films(sc, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for i in range(2):
        sc.render_into(*films, i, i + 1, 5, st)
    torch.cuda.synchronize(dev)
    ratios = []
    for i in range(2, 6):
        t0 = time.perf_counter()
        sc.render_async_into(*films, i, i + 1, 5, st)
        t1 = time.perf_counter()
        sc.join(st)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        ratios.append((t1 - t0) / (t2 - t0))
    print("enqueue / pass:", ["%.3f" % r for r in ratios])
    assert sorted(ratios)[1] < 0.35, ratios


def test_progressive_render_progress_and_cancel(built):
    """wtgpu_render_progressive / wtgpu_cancel (scene_renderer.hpp:42-62): the callback sees every chunk; stopping after chunk k leaves
    exactly k chunks in the films (= the joined render of those samples); a cancel from another thread does the same."""
    import threading
    import torch
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.render import alloc_films
    sc = Scene("furnace", res=32, lut=(32, 32))
    sc.upload(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    seen = []
    v, w, l = alloc_films(sc, dev)
    cancelled, done = sc.render_progressive(v, w, l, 0, 6, 21, chunk_spp=2, progress=lambda d, t: seen.append((d, t)) or False, stream=st)
    assert not cancelled and done == 6 and seen == [(2 * 1024, 6 * 1024), (4 * 1024, 6 * 1024), (6 * 1024, 6 * 1024)]
    ref = render(sc, 6, seed=21)
    assert np.allclose(v.cpu().numpy(), ref[0], rtol=1e-9, atol=1e-30)
    # stop from the callback after the second chunk
    v, w, l = alloc_films(sc, dev)
    cancelled, done = sc.render_progressive(v, w, l, 0, 6, 21, chunk_spp=1, progress=lambda d, t: d >= 2 * 1024, stream=st)
    assert cancelled and done == 2
    ref2 = render(sc, 2, seed=21)
    assert np.allclose(v.cpu().numpy(), ref2[0], rtol=1e-9, atol=1e-30) and np.allclose(w.cpu().numpy(), ref2[1], rtol=1e-12)
    # cancel from another thread while a long render is running
    v, w, l = alloc_films(sc, dev)
    t = threading.Timer(0.05, sc.cancel)
    t.start()
    cancelled, done = sc.render_progressive(v, w, l, 0, 100000, 21, chunk_spp=1, stream=st)
    t.join()
    assert cancelled and 0 < done < 100000
    refd = render(sc, done, seed=21)                                            # exactly `done` complete chunks are in the films
    assert np.allclose(w.cpu().numpy(), refd[1], rtol=1e-12) and np.allclose(v.cpu().numpy(), refd[0], rtol=1e-9, atol=1e-30)


def test_rccl_film_reduce_world_size_1(built):
    """wtgpu_comm_* / wtgpu_film_reduce (RCCL) at world size 1: the library's own collective path initialises and leaves the films
    unchanged; render_distributed over torch.distributed's nccl backend gives the single-process render."""
    import os
    import torch
    import torch.distributed as dist
    from wave_tracer_amd import Scene, render
    from wave_tracer_amd.api import Comm
    from wave_tracer_amd.render import alloc_films, make_film_comm, render_distributed
    sc = Scene("furnace", res=24, lut=(32, 32))
    sc.upload(0)
    ref = render(sc, 4, seed=3)
    dev = torch.device("cuda", 0)
    v, w, l = alloc_films(sc, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    sc.render_into(v, w, l, 0, 4, 3, st)
    comm = Comm(1, 0, 0, Comm.unique_id())
    comm.film_reduce(v, w, l, root=0, stream=st)
    torch.cuda.synchronize(dev)
    comm.close()
    assert np.allclose(v.cpu().numpy(), ref[0], rtol=1e-9, atol=1e-30) and np.allclose(w.cpu().numpy(), ref[1], rtol=1e-12)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        out = render_distributed(sc, 4, seed=3)
        c2 = make_film_comm(0)   # the path bench.py --gpus N takes: id over torch.distributed, reduce inside the C-ABI
        out2 = render_distributed(sc, 4, seed=3, comm=c2)
        c2.close()
    finally:
        dist.destroy_process_group()
    assert np.allclose(out[0], ref[0], rtol=1e-9, atol=1e-30) and np.allclose(out[2], ref[2], rtol=1e-9, atol=1e-30)
    assert np.allclose(out2[0], ref[0], rtol=1e-9, atol=1e-30) and np.allclose(out2[2], ref[2], rtol=1e-9, atol=1e-30)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["furnace", "etoile"])
def test_two_ranks_one_gpu_sharded_render(built, tmp_path, name):
    """render_distributed with the PRODUCT shard renderer (HIP) on two ranks that share the box's GPU (gloo: the films are summed over the
    host): the reduced film equals the single-process render of the whole sample range — sample-index sharding, disjoint Philox streams
    per shard, additive films — for plt_bdpt and for the forward plt_path scene."""
    import os
    import socket
    import subprocess
    import sys
    from wave_tracer_amd import Scene, render
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "dist_hip.npz")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_KERNARG_POOL_SIZE=str(16 << 20))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(here, "_dist_worker_hip.py"), out, "6", "17", name]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    sc = Scene(name, res=24, lut=(32, 32), mesh_detail=0)
    v, w, l = render(sc, 6, seed=17)
    assert v.sum() + l.sum() > 0
    # (f64 atomics: the order of the film sums differs between one process and two)
    assert np.allclose(d["value"], v, rtol=1e-9, atol=1e-30) and np.allclose(d["weight"], w, rtol=1e-9) and np.allclose(d["light"], l, rtol=1e-9, atol=1e-30)


def test_bench_launches_its_own_ranks(built):
    """`python bench.py --gpus N` with no launcher around it (the driver's N = 1 form, and what a user types) starts N ranks itself and
    rank 0 prints ONE JSON line with n_gpus = N.  Two ranks share the box's single GPU here (--backend gloo: the film reduce goes over
    the host; the RCCL path needs one GPU per rank)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1",
                                   "--scene", "furnace", "--res", "64", "--spp-per-step", "1", "--no-cpu-baseline", "--no-traffic"], env=env, stderr=subprocess.DEVNULL).decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["samples_per_step"] == 64 * 64 and abs(d["value"] - 2 * 2 * 64 * 64 / (d["ms_per_step"] * 2e-3) / 1e6) < 1e-6 * d["value"]
    assert "roofline" in d and "whole_path" in d["roofline"]


def test_bench_full_adds_the_cpu_baseline(built):
    """A plain `bench.py` run reports the headline and the roofline of its own counters only; `--full` adds the legs that take runs of
    their own (here the CPU baseline; the live PMC passes are skipped with --no-traffic)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--scene", "furnace", "--res", "64", "--spp-per-step", "1"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-traffic", "--cpu-seconds", "1"])):
        out = subprocess.check_output(common + extra, env=env, stderr=subprocess.DEVNULL, timeout=300).decode()
        ls = [l for l in out.splitlines() if l.startswith("{")]
        assert len(ls) == 1, out
        lines[name] = json.loads(ls[0])
    for d in lines.values():
        assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["unit"] == "Msamples/s" and d["higher_is_better"]
        assert d["config"]["samples_per_step"] == 64 * 64 and "whole_path" in d["roofline"]
    assert "cpu_baseline" not in lines["plain"]
    assert (lines["plain"]["roofline"]["traffic_source"] or {}).get("measured") is None
    cb = lines["full"]["cpu_baseline"]
    assert cb["value"] > 0 and cb["unit"] == "Msamples/s" and cb["cores"] >= 1


def test_pause_resume_and_capture_intermediate(built):
    """The renderer's remaining interrupts (include/wt/scene/interrupts.hpp; src/scene/render.cpp:306-368) at the C-ABI: a pause requested from
    the progress callback holds the render at the chunk boundary while another thread asks for an intermediate capture (served WHILE paused, with
    the films holding exactly the completed chunks: they equal a direct render of those samples), then resumes it; the finished film equals an
    uninterrupted render."""
    import threading
    import time
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    sc = Scene("furnace", res=48)
    sc.upload(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ref = alloc_films(sc, dev)
    sc.render_into(*ref, 0, 12, 21, st)
    part = alloc_films(sc, dev)
    sc.render_into(*part, 0, 4, 21, st)
    torch.cuda.synchronize(dev)
    films = alloc_films(sc, dev)
    seen = {}

    def capture(done):
        torch.cuda.synchronize(dev)
        seen["done"] = done
        seen["value"] = films[0].clone()
        seen["t"] = time.monotonic()

    def helper():                       # another thread: waits until the render is paused, captures, then resumes it
        while "paused_at" not in seen:
            time.sleep(0.002)
        sc.capture_intermediate(capture)
        while "done" not in seen:
            time.sleep(0.002)
        time.sleep(0.05)
        seen["resumed_at"] = time.monotonic()
        sc.resume()

    def progress(done, total):
        if done == 4 * 48 * 48 and "paused_at" not in seen:
            sc.pause()
            seen["paused_at"] = time.monotonic()
        seen.setdefault("calls", []).append((done, time.monotonic()))
        return False
    th = threading.Thread(target=helper)
    th.start()
    cancelled, spe = sc.render_progressive(*films, 0, 12, 21, chunk_spp=4, progress=progress, stream=st)
    th.join(10)
    torch.cuda.synchronize(dev)
    assert not cancelled and spe == 12
    assert seen["done"] == 4 and torch.allclose(seen["value"], part[0], rtol=1e-12, atol=0)   # captured while paused: exactly the first chunk
    later = [t for d, t in seen["calls"] if d > 4 * 48 * 48]
    assert len(later) == 2 and min(later) >= seen["resumed_at"]                             # nothing was launched before the resume
    for a, b in zip(films, ref):
        assert torch.allclose(a, b, rtol=1e-12, atol=0)
    # a capture requested while no render runs is served at the next render's first boundary; a pause with a cancel ends the render
    sc.capture_intermediate(lambda d: seen.__setitem__("late", d))
    sc.pause()
    threading.Timer(0.05, sc.cancel).start()
    cancelled, spe = sc.render_progressive(*alloc_films(sc, dev), 0, 8, 3, chunk_spp=2, stream=st)
    sc.resume()
    assert cancelled and spe == 2 and seen["late"] == 2


def test_render_with_preview_on_the_gpu(built):
    """§8f N4 on hardware: render_with_preview drives wtgpu_render_progressive and pushes the developed partial film to a tev viewer (here the
    local stand-in of tests/test_preview.py): one CreateImage, updates while the render runs, the last update = the finished, developed film."""
    from test_preview import _FakeTev, _parse
    from wave_tracer_amd import Scene, develop
    from wave_tracer_amd.preview import TevPreview, render_with_preview
    srv = _FakeTev()
    pv = TevPreview("127.0.0.1", srv.port, min_interval_s=0.0)
    sc = Scene("furnace", res=40)
    v, w, l = render_with_preview(sc, 12, pv, seed=5, chunk_spp=4, preview_id="camera")
    pv.close()
    srv.join(5.0)
    pk = _parse(srv.data)
    assert [k[0] for k in pk] == ["create", "update", "update", "update"] and all(k[1] == "wave_tracer 'camera'" for k in pk)
    assert pk[0][3:5] == (sc.width, sc.height)
    final = develop(sc, v, w, l, 12).reshape(sc.height, sc.width, -1)
    shown = pk[-1][7].reshape(3, sc.height, sc.width)
    rgb = np.repeat(final, 3, axis=-1)[..., :3] if final.shape[-1] == 1 else final[..., :3]
    assert np.allclose(shown, np.moveaxis(rgb, -1, 0), rtol=1e-6, atol=0)
    ov, ow, ol, _ = oracle_render(sc, 0, 12, 5)
    parity.check("render_with_preview", _rel_l1(final, develop(sc, ov, ow, ol, 12).reshape(final.shape)), 1e-2)


def test_two_gpus_strong_scaling_through_rccl(built):
    """The multi-GPU path on real hardware, wherever the box has two GPUs (skipped on the one-GPU boxes of this round): `bench.py --gpus 2
    --backend nccl --scaling strong` — two ranks, one GPU each, every rank renders half of the samples of every step, the films are reduced
    by wtgpu_film_reduce (one ncclGroup of three ncclReduce over RCCL).  With --warmup 0 the two ranks render exactly the samples a single rank
    renders with the same --spp-per-step: the reduced film must equal the single-rank film (f64 atomics: to rounding)."""
    import json
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = ["--steps", "3", "--warmup", "0", "--scene", "cornell_box", "--res", "256", "--spp-per-step", "2", "--no-cpu-baseline", "--no-traffic", "--film-sums"]

    def run(extra):
        out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py")] + extra + common, env=env, stderr=subprocess.DEVNULL).decode()
        lines = [l for l in out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out
        return json.loads(lines[0])
    two = run(["--gpus", "2", "--backend", "nccl", "--scaling", "strong"])
    one = run(["--gpus", "1"])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["film_reduce"]["ranks"] == 2 and "RCCL" in two["film_reduce"]["through"]
    assert two["film_reduce"]["rccl_version"] and len(two["per_rank"]) == 2
    assert two["config"]["samples_per_step"] == one["config"]["samples_per_step"] == 2 * 256 * 256
    for k in ("value", "weight", "light"):
        a, b = two["film_sums"][k], one["film_sums"][k]
        assert abs(a - b) <= 1e-9 * abs(b) + 1e-30, (k, a, b)


@pytest.mark.gpu
def test_two_ranks_strong_scaling_through_gloo_on_one_gpu(built):
    """The same driver line (`bench.py --gpus 2 --scaling strong`) where only ONE GPU is visible: two ranks share it, the films travel through
    gloo instead of RCCL (--backend gloo).  Everything but the collective is the multi-GPU path — sample-index sharding, per-rank films, the
    reduce onto rank 0, the max-over-ranks clock — and the line carries what makes a first real 8-GPU run self-diagnosing: per-rank rates, the
    reduce's byte count, the backend."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = ["--steps", "3", "--warmup", "0", "--scene", "cornell_box", "--res", "128", "--mesh-detail", "0", "--spp-per-step", "2", "--no-cpu-baseline", "--no-traffic", "--film-sums"]

    def run(extra):
        out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py")] + extra + common, env=env, stderr=subprocess.DEVNULL, timeout=300).decode()
        lines = [l for l in out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out
        return json.loads(lines[0])
    two = run(["--gpus", "2", "--backend", "gloo", "--scaling", "strong"])
    one = run(["--gpus", "1"])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["film_reduce"]["ranks"] == 2 and two["film_reduce"]["backend"] == "gloo"
    assert two["film_reduce"]["bytes_per_rank"] == 128 * 128 * 8 * (3 + 1 + 3)
    assert len(two["per_rank"]) == 2 and all(r["msamples_per_s"] > 0 for r in two["per_rank"])
    assert two["config"]["samples_per_step"] == one["config"]["samples_per_step"] == 2 * 128 * 128
    for k in ("value", "weight", "light"):
        a, b = two["film_sums"][k], one["film_sums"][k]
        assert abs(a - b) <= 1e-9 * abs(b) + 1e-30, (k, a, b)


def test_converged_bias_dense_crop(built):
    """BASELINE.json's second metric: converged-image error against the CPU reference (north_star: < 1e-3).  Dense-mesh crop of the
    headline film (same pixel pitch as the 1440^2 render).
    (1) PAIRED estimate of the bias (common random numbers: both sides consume identical Philox streams, so the difference of the
        film sums is carried by the few samples that differ — a low-variance estimate of E[gpu] - E[cpu]), 256 spp in 16 chunks.
        Asserted on ALL cells, nothing trimmed: |sum_gpu - sum_cpu| < 1e-3 sum_cpu and within 3 bootstrap standard errors (+ 1e-4) of
        zero; the (pixel, chunk) cells that hold a sample on a different discrete path ("divergent": the two sums differ by more than half)
        are < 0.1 % of the cells and, when there are at least 6 of them, sign-balanced (two-sided binomial p > 0.01).
        History: round 2 measured +2.35e-2 over all cells with 11 divergent cells, all GPU-larger.  The cause was fused multiply-add
        contraction: hipcc and g++ contracted different expressions of the shared headers, and the estimator's discontinuities (a
        Fraunhofer pdf is clamped to zero at 100 sr^-1, free_space_diffraction.hpp:133; a pdf <= FLT_EPSILON counts as 1 in the MIS sums,
        plt_bdpt_detail.hpp:688-719) turned last-bit differences of 1 - flux into one-sided firefly-weighted flips.  Both sides are now
        built with -ffp-contract=off (explicit fmaf stays): measured -3e-6 +- 8e-6 at 256 spp, -9e-6 +- 2e-5 at 1024 spp with ONE
        divergent cell in 65,536 (tools/paired_bias.py, gpurun_out/r3n).
    (2) INDEPENDENT seeds at 1024 spp: GPU(seed A) against the CPU checker(seed C), judged against the Monte-Carlo floor measured
        by two GPU renders with different seeds (A, B): block means and the crop mean agree within the floor.
    Prints all numbers."""
    from wave_tracer_amd import Scene, render, develop
    from oracle_util import paired_bias_stats
    kw = dict(mesh_detail=1, lut=(128, 128), crop_of=1440)
    res = 32
    sc = Scene("cornell_box", res=res, **kw)
    # (1) paired
    G, C = [], []
    for chunk in range(16):
        b, e = chunk * 16, (chunk + 1) * 16
        v, w, l = render(sc, e - b, seed=31, sample_begin=b)
        ov, ow, ol, _ = oracle_render(sc, b, e, 31)
        G.append(v.sum(axis=2) + l.sum(axis=2))
        C.append(ov.sum(axis=2) + ol.sum(axis=2))
    st = paired_bias_stats(np.array(G), np.array(C))
    print(f"paired bias, 256 spp: all cells {st['bias_all']:+.2e} +- {st['se_all']:.1e}; {st['n_div']} of {len(G) * res * res} cells diverge discretely "
          f"({st['n_pos']} GPU-larger, sign p = {st['p_sign']:.3f}); non-divergent cells {st['bias_trim']:+.2e} +- {st['se_trim']:.1e}, rel L1 {st['rel_l1_trim']:.2e}")
    assert abs(st["bias_all"]) < 1e-3 and abs(st["bias_all"]) < 3 * st["se_all"] + 1e-4, st
    assert abs(st["bias_trim"]) < 1e-3, st
    assert st["frac_div"] < 1e-3 and (st["n_div"] < 6 or st["p_sign"] > 0.01), st
    # ... and against the checker running the interaction records AS EXECUTED by the reference (the final-slab filter never fires there:
    # src/ads/bvh8w.cpp:175 records no distance) instead of as written: the one known semantic deviation of this path.
    # CPU-only measurement at 1024 spp (tools/filter_effect.py): as executed - as written = -2.8e-4 +- 1.6e-4 of the crop's flux (+2.7 %
    # Fraunhofer interactions), 1e-8 on the double slits.  Here: the GPU stays within the 1e-3 tolerance of that variant too.
    from oracle_util import load_oracle
    lib = load_oracle()
    C0 = []
    lib.oracle_set_region_filter(0)
    try:
        for chunk in range(16):
            ov, ow, ol, _ = oracle_render(sc, chunk * 16, (chunk + 1) * 16, 31)
            C0.append(ov.sum(axis=2) + ol.sum(axis=2))
    finally:
        lib.oracle_set_region_filter(1)
    st0 = paired_bias_stats(np.array(G), np.array(C0))
    print(f"against the as-executed records: all cells {st0['bias_all']:+.2e} +- {st0['se_all']:.1e}, {st0['n_div']} divergent cells")
    assert abs(st0["bias_all"]) < 1e-3 + 3 * st0["se_all"], st0

    # (2) independent seeds
    def blocks(img):
        return img.reshape(res // 8, 8, res // 8, 8, -1).sum(axis=(1, 3, 4))
    spp = 1024
    imgs = []
    for seed in (101, 202):
        v, w, l = render(sc, spp, seed=seed)
        imgs.append(develop(sc, v, w, l, spp).astype(np.float64))
    ov, ow, ol, _ = oracle_render(sc, 0, spp, 303)
    c = develop(sc, ov, ow, ol, spp).astype(np.float64)
    ba, bb, bc = blocks(imgs[0]), blocks(imgs[1]), blocks(c)
    floor_rms = float(np.sqrt(np.mean((ba - bb) ** 2)) / bc.mean())
    d_rms = float(np.sqrt(np.mean((ba - bc) ** 2)) / bc.mean())
    print(f"independent seeds, {spp} spp: normalised RMSE of 8x8 block means GPU vs CPU {d_rms:.3e}, GPU vs GPU floor {floor_rms:.3e}; "
          f"crop mean GPU {imgs[0].mean():.6g} / {imgs[1].mean():.6g} CPU {c.mean():.6g}")
    # medians are robust against the fireflies that dominate the means at this sample count
    med = [np.median(x.sum(axis=2)) for x in (imgs[0], imgs[1], c)]
    print(f"median pixel value GPU {med[0]:.6g} / {med[1]:.6g} CPU {med[2]:.6g}")
    assert d_rms < 3.0 * floor_rms + 1e-3, (d_rms, floor_rms)
    assert abs(med[0] - med[2]) <= 3 * abs(med[0] - med[1]) + 5e-3 * med[2]


def test_full_size_etoile_720(built):
    """BASELINE.json configs[3] at its full film size: the etoile stand-in at the complexity SURVEY.md §8(d) C4 prescribes (ground + 576 seeded
    buildings + the arch, 5 ITU materials: mesh_detail = 2), 720 x 540, 10 GHz, forward plt_path with UTD.  Forward samples splat anywhere on
    the film, so the comparison is of WHOLE films: the GPU's 2 spp against the CPU checker's same 2 spp (777,600 samples) — film sums to
    1e-3, developed image rel. L1 < 2e-2, event counters 0.5 % — plus finiteness, non-negativity and film linearity."""
    import torch
    from wave_tracer_amd import Scene, develop
    from wave_tracer_amd.render import alloc_films
    sc = Scene("etoile", res=720, mesh_detail=2)
    assert (sc.width, sc.height) == (720, 540) and sc.info.n_shapes > 560 and int(sc.info.integrator) == 1
    sc.upload(0, 720 * 540)
    dev = torch.device("cuda", 0)
    films = [alloc_films(sc, dev) for _ in range(3)]
    st = torch.cuda.current_stream(dev).cuda_stream
    sc.reset_counters()
    sc.render_into(*films[0], 0, 1, 5, st)
    sc.render_into(*films[1], 1, 2, 5, st)
    c = sc.counters()
    sc.render_into(*films[2], 0, 2, 5, st)
    torch.cuda.synchronize(dev)
    for v, w, l in films:
        assert torch.isfinite(v).all() and torch.isfinite(l).all() and (l >= 0).all() and (v >= 0).all()
    for k in range(3):
        assert torch.allclose(films[0][k] + films[1][k], films[2][k], rtol=1e-7, atol=1e-30)
    assert c["samples"] == 2 * 720 * 540 and c["walk_iteration_cap_hits"] == 0 and c["traversal_stack_dropped"] == 0
    ov, ow, ol, oc = oracle_render(sc, 0, 2, 5)
    g = develop(sc, *(t.cpu().numpy() for t in films[2]), 2).astype(np.float64)
    cpu = develop(sc, ov, ow, ol, 2).astype(np.float64)
    gl = films[2][2].cpu().numpy()
    print("etoile 720x540:", "film sum GPU", gl.sum(), "CPU", ol.sum(), "rel L1", _rel_l1(g, cpu), {k: (c[k], oc[k]) for k in ("segments", "fsd_interactions", "light_splats", "shadow_rays")},
          "overflows", {k: c[k] for k in ("cone_tri_overflow", "edge_overflow", "fsd_edge_overflow")})
    assert cpu.sum() > 0
    parity.check("full_size_etoile_720/film_sum", abs(gl.sum() - ol.sum()) / ol.sum(), 1e-3)
    parity.check("full_size_etoile_720/image", _rel_l1(g, cpu), 2e-2)
    # classified-edge sets and wedge lists are complete (k_path_edges + the per-round wedge pools): nothing truncated, like the reference's vectors
    assert c["edge_overflow"] == 0 and c["fsd_edge_overflow"] == 0 and c["fsd_pool_overflow"] == 0
    for key in ("segments", "fsd_interactions", "light_splats"):
        assert abs(c[key] - oc[key]) <= 5e-3 * oc[key], (key, c[key], oc[key])


def test_full_size_bidir_room_1920_polarimetric(built):
    """BASELINE.json configs[4] at its full film size: the bidir_room stand-in at the complexity SURVEY.md §8(d) C5 prescribes (room + 51
    objects, 21 diffuse / 9 surface_spm / 4 dielectric materials: mesh_detail = 2), 1920 x 1088, polarimetric film (4 Stokes components per
    RGB channel), plt_bdpt.  Size-independent properties (finite films, non-negative intensity planes, one unit of reconstruction weight
    per sample, |Q|,|U|,|V| <= I on the accumulated film up to noise is NOT a per-pixel invariant and is not asserted, linearity) and
    sample-for-sample parity with the CPU checker on every 97th 24x24 block of the same film (value / weight planes of the pixels
    inside those blocks)."""
    import torch
    from oracle_util import oracle_render_tiles
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    sc = Scene("bidir_room", res=1920, mesh_detail=2, polarimetric=1)
    assert (sc.width, sc.height, sc.channels) == (1920, 1088, 12) and sc.info.n_shapes >= 50 and sc.info.n_materials == 34
    npix = 1920 * 1088
    sc.upload(0, npix)
    dev = torch.device("cuda", 0)
    films = [alloc_films(sc, dev) for _ in range(3)]
    st = torch.cuda.current_stream(dev).cuda_stream
    sc.reset_counters()
    sc.render_into(*films[0], 0, 1, 5, st)
    sc.render_into(*films[1], 1, 2, 5, st)
    c = sc.counters()
    sc.render_into(*films[2], 0, 2, 5, st)
    torch.cuda.synchronize(dev)
    for v, w, l in films:
        assert torch.isfinite(v).all() and torch.isfinite(w).all() and torch.isfinite(l).all()
        assert (v.reshape(1088, 1920, 3, 4)[..., 0] >= 0).all() and (w >= 0).all() and (l.reshape(1088, 1920, 3, 4)[..., 0] >= 0).all()
    wsum = float(films[0][1].sum())
    assert 0.995 * npix < wsum <= npix * (1 + 1e-6), wsum / npix
    for k in range(3):
        assert torch.allclose(films[0][k] + films[1][k], films[2][k], rtol=1e-7, atol=1e-30)
    # (the walk-iteration cap — 96 trace/interact rounds per subpath, the CPU checker's too; the reference recurses without one — is reached by
    # a few walks in 10^6 here: beams that restart behind empty apertures over and over)
    assert c["samples"] == 2 * npix and c["walk_iteration_cap_hits"] == 0 and c["fsd_pool_overflow"] == 0 and c["traversal_stack_dropped"] == 0
    ov, ow, ol, oc5, n5, mask = oracle_render_tiles(sc, 0, 1, 5, 97)
    inner = mask.copy()
    inner[1:, :] &= mask[:-1, :]
    inner[:-1, :] &= mask[1:, :]
    inner[:, 1:] &= mask[:, :-1]
    inner[:, :-1] &= mask[:, 1:]
    inner[0, :] = inner[-1, :] = inner[:, 0] = inner[:, -1] = False
    gv, gw = films[0][0].cpu().numpy(), films[0][1].cpu().numpy()
    assert inner.sum() > 15000
    assert np.allclose(gw[inner], ow[inner], rtol=1e-5, atol=1e-7)
    rel = np.abs(gv[inner] - ov[inner]).sum() / np.abs(ov[inner]).sum()
    frac_same = (np.abs(gv[inner] - ov[inner]).sum(axis=1) <= 1e-3 * np.abs(ov[inner]).sum(axis=1) + 1e-30).mean()
    print("iteration cap hits", c["walk_iteration_cap_hits"], "of", c["samples"])
    print("bidir_room 1920x1088 polarimetric: rel L1", rel, "frac_same", frac_same, "fsd", c["fsd_interactions"], "overflows",
          {k: c[k] for k in ("edge_overflow", "fsd_edge_overflow", "fsd_pool_overflow")})
    parity.check("full_size_bidir_room_1920_polarimetric/blocks_value", rel, 2e-2)
    assert frac_same > 0.99, frac_same


def test_c1_against_the_committed_cpu_record(built):
    """BASELINE.json configs[0] (C1: cornell-box res 256, spp 64): the GPU render of the very samples of the CPU checker's committed record
    (profiles/r04_cpu_c1_record.json, tools/cpu_c1_record.py: seed 1, samples [0, 64)) — film sums to 2e-3 (a few samples in 10^3 take another
    discrete path on the GPU: DESIGN.md section 5), event statistics per sample to 0.5 %, weights to 1e-5."""
    import json
    import os
    from wave_tracer_amd import Scene, render
    rec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r04_cpu_c1_record.json")))
    sc = Scene("cornell_box", res=256, mesh_detail=1)
    sc.upload(0)
    sc.reset_counters()
    v, w, l = render(sc, 64, seed=1)
    c = sc.counters()
    n = sc.width * sc.height * 64
    assert rec["samples"] == n == c["samples"]
    fs = rec["film_sums"]
    assert abs(w.sum() / fs["weight"] - 1) < 1e-5
    assert abs(v.sum() / fs["value"] - 1) < 2e-3 and abs(l.sum() / fs["light"] - 1) < 2e-3, (v.sum() / fs["value"], l.sum() / fs["light"])
    for k in ("segments", "vertices", "connections"):
        assert abs(c[k] / n / rec["counters_per_sample"][k] - 1) < 5e-3, (k, c[k] / n, rec["counters_per_sample"][k])
    assert c["walk_iteration_cap_hits"] == 0 and c["traversal_stack_dropped"] == 0
