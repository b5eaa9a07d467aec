"""The device's region power integral: query by query (wtgpu_test_flux_queries, kernels_test.hip: k_test_flux; wt/flux_probe.h) on the sets of
tests/test_flux_probe.py against the CPU checker's twin and the f64 reference (oracle/flux64.cpp), whole regions (wtgpu_query_regions:
coop_gather) against the f64 sum over the checker's triangle ids, and the subtree tasks of a render (k_flux_split / k_flux_tasks) at two task
sizes.

Bounds.  Every word that involves only + - x /, sqrtf and comparisons is bit-identical to the twin (both sides are compiled with
-ffp-contract=off).  The flux words and the intensity, which sit behind expf / logf / atan2f / cosf of two different maths libraries, are
held per class to |device - ref| <= 4 x the committed twin/<class> error + 1e-7 (tests/golden/flux_measured.json) and always to the CPU
test's bound: both sides evaluate the same ~150 transcendentals per triangle and both libraries are good to 1 - 2 ulp, so a device error
several times the twin's means that one call is wrong, not rounding.  PARITY_RECORD=1 also writes the device's worst error per class to
the record directory of tests/parity.py (flux_measured.json) as device/<class> (kept for information; it is not the tolerance).

Measured on the MI355X (device/<class> of the committed file; twin in brackets): between 0.89 and 1.36 x the twin's worst error in every class,
e.g. gauss_s3 2.03e-7 (1.68e-7), gauss_s8 4.05e-7 (3.99e-7), gauss_scale50 1.97e-6 (2.03e-6), gauss_switch 1.90e-8 (1.40e-8), region_local_*
6.0e-7 .. 9.3e-7 (6.0e-7 .. 9.0e-7), region_tuid 1.74e-6 (1.74e-6), wavefront 2.62e-7 (2.48e-7), the intensity 1.64e-6 relative (1.64e-6);
whole regions 8.52e-5 (8.53e-5), above 2000 triangles 1.38e-7 (1.38e-7); 848,383 words bit-identical."""
import numpy as np
import pytest

import flux_probe as fp
from test_gpu_traversal import oracle_regions

pytestmark = pytest.mark.gpu

LIBM_WORDS = {fp.GAUSS: (fp.W_FLUX,), fp.WAVEFRONT: (fp.W_FLUX, fp.W_AUX), fp.REGION_LOCAL: (fp.W_FLUX,), fp.REGION_TUID: (fp.W_FLUX,)}


@pytest.fixture(scope="module")
def dev_sets(built):
    from wave_tracer_amd import Scene
    sc, qs = fp.flux_sets(Scene)
    sc.upload(0)
    out = {}
    for name, (q, cls, info) in qs.items():
        twin = fp.oracle_flux_queries(sc, q)
        out[name] = (q, cls, info, sc.flux_queries(q), twin, fp.reference(sc, q, twin))
    return sc, out


def test_device_words_identical_to_the_twin(dev_sets):
    """the branch word, `tris`, the five clipped vertices, the projected vertices, the beam-frame vertices and the facing bit: the same bits (signed
    zeros included); a difference names the first differing query and word"""
    n_words = 0
    for name, (q, cls, info, dev, twin, ref) in dev_sets[1].items():
        exact = np.ones(fp.OW, bool)
        exact[list(LIBM_WORDS[int(q[0, 0])])] = False
        diff = np.argwhere(dev[:, exact] != twin[:, exact])
        if len(diff):
            i, w = int(diff[0, 0]), int(np.nonzero(exact)[0][diff[0, 1]])
            raise AssertionError(f"{name}: {len(diff)} words differ; first: query {i} ({cls[i]}), word {w}: device {dev[i, w]:#010x} twin {twin[i, w]:#010x} "
                                 f"({dev[i, w:w + 1].view(np.float32)[0]!r} vs {twin[i, w:w + 1].view(np.float32)[0]!r}); query words {q[i].tolist()}")
        n_words += int(exact.sum()) * len(q)
    print(f"device vs twin: {n_words} words compared bit for bit")
    assert n_words > 500000


def test_device_flux_against_f64(dev_sets):
    """per class: |device - ref| <= 4 x the committed twin error + 1e-7 and within the CPU bound (2e-6 + 1e-5 ref; scale 50: 2 x its committed
    twin error; the intensity: relative, within its rounding unit); finite, in [0, 1]; the exact zeros and the inf of a vanishing sigma"""
    committed = fp.measured()
    worst = {}
    for name, (q, cls, info, dev, twin, ref) in dev_sets[1].items():
        got = fp.out_flux(dev)
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), name
        err = np.abs(got - ref["flux"])
        worst.update(fp.class_errors(cls, err))
        cpu = np.where(cls == "gauss_scale50", 2 * committed["twin/gauss_scale50"], fp.cpu_bound(ref["flux"]))
        bad = np.nonzero(err > cpu)[0]
        assert not len(bad), (name, len(bad), [(int(i), cls[i], got[i], ref["flux"][i]) for i in bad[:5]])
        # the exact zeros: zero area, a vanishing sigma, wholly outside the slab, the wrong facing
        zero = {"gauss": np.isin(np.arange(len(q)), info.get("zero_area", [])), "wavefront": cls == "wavefront_zero_sigma",
                "region_local": info.get("kind", cls) == "outside", "region_tuid": dev[:, fp.W_AUX] != q[:, 18]}[name]
        assert zero.sum() >= 12 and (dev[zero, fp.W_FLUX] == 0).all(), name
        if name == "wavefront":
            m = cls == "wavefront"
            inten = fp.floats(dev[m, fp.W_AUX])
            rel = np.abs(inten - ref["aux"][m]) / ref["aux"][m]
            assert np.isfinite(inten).all() and (rel <= fp.intensity_unit(q[m])).all(), float((rel / fp.intensity_unit(q[m])).max())
            worst["wavefront_intensity"] = float(rel.max())
            assert (dev[~m, fp.W_AUX] == twin[~m, fp.W_AUX]).all()                   # inf on the axis, 0 off it
    for k, v in sorted(worst.items()):
        print(f"device/{k}: {v:.3e}   (twin/{k}: {committed['twin/' + k]:.3e})")
    if fp.recording():
        fp.record({f"device/{k}": v for k, v in worst.items()})
    assert len(worst) >= 18
    for k, v in worst.items():
        assert v <= 4 * committed[f"twin/{k}"] + 1e-7, (k, v, committed[f"twin/{k}"])


def test_tail_of_the_last_block(dev_sets):
    """launches of 1, 63, 64, 65 queries write the same rows as the full set"""
    sc, sets = dev_sets
    for name in ("gauss", "region_local"):
        q, full = sets[name][0], sets[name][3]
        for n in (1, 63, 64, 65):
            assert np.array_equal(sc.flux_queries(q[100:100 + n]), full[100:100 + n]), (name, n)


def test_invalid_queries_are_rejected(dev_sets):
    """an op outside the table or a tuid >= the scene's triangle count returns WTGPU_ERR_INVALID and launches nothing"""
    sc, sets = dev_sets
    good = sets["region_tuid"][0][:3]
    bad_tuid, bad_op = good[0].copy(), good[0].copy()
    bad_tuid[17] = sc.info.n_tris
    bad_op[0] = len(fp.OPS)
    for bad in (bad_tuid, bad_op):
        with pytest.raises(Exception, match="wtgpu error 1.*out of range"):
            sc.flux_queries(np.concatenate([good, bad[None]]))
    assert np.array_equal(sc.flux_queries(good), sets["region_tuid"][3][:3])      # the scene still answers


def test_whole_regions_against_the_f64_sum(built):
    """wtgpu_query_regions (coop_gather: f32 contributions, f64 butterfly sum) on the bench geometry against ref_region_sum over the checker's
    triangle ids (the unbounded record after the final-slab filter), for the regions whose device triangle count equals the checker's (>= 95 % of
    the non-ballistic ones): |device - ref| <= 4 x the twin's worst |slab flux - ref| on the same regions + 1e-7, and the 1e-3 of
    test_whole_region_queries_beyond_the_list_cap on all of them.
    Cones: flux_probe.whole_region_cones (region_cones(120, 18) hold only 2 regions of more than 2000 triangles; 120 more of the family: 10).
    The twin's worst error here (8.5e-5, on a region of one triangle; 1.4e-7 on the regions above 2000 triangles, which are held to 4 x that
    on their own) is the conditioning of the f32 change to the beam frame (a 10-um beam 20 mm from its origin: 1e-9 m is 1e-4 sigma), which
    the device shares bit for bit."""
    from wave_tracer_amd import Scene
    sc = fp.whole_region_scene(Scene)
    sc.upload(0)
    cones = fp.whole_region_cones()
    g, o = sc.query_regions(cones), oracle_regions(sc, cones)
    ntris, ref = fp.region_reference(sc, cones)
    diff = (o["flags"] & 3) == 0
    assert (g["flags"] == o["flags"]).all() and (ntris[diff] == o["ntris"][diff, 0]).all() and (o["ntris"][diff, 0] == o["ntris"][diff, 1]).all()
    same = diff & (g["ntris"] == o["ntris"][:, 1])
    assert same.sum() >= 0.95 * diff.sum(), (int(same.sum()), int(diff.sum()))
    assert (ntris[same] > 64).sum() >= 20 and (ntris[same] > 2000).sum() >= 5, ((ntris[same] > 64).sum(), (ntris[same] > 2000).sum())
    twin = np.abs(o["flux"][same, 1].astype(np.float64) - ref[same])
    dev = np.abs(g["flux"][same].astype(np.float64) - ref[same])
    big = ntris[same] > 2000
    print(f"whole regions: {int(same.sum())} of {int(diff.sum())} compared, {int((ntris[same] > 64).sum())} above 64 triangles, {int(big.sum())} above 2000 "
          f"(largest {int(ntris[same].max())}); worst |flux - f64 sum|: device {dev.max():.3e}, twin {twin.max():.3e}; above 2000 triangles: device "
          f"{dev[big].max():.3e}, twin {twin[big].max():.3e}; device vs twin {np.abs(g['flux'][same] - o['flux'][same, 1]).max():.3e}")
    if fp.recording():
        fp.record({"device/region_sum": dev.max()})
    assert dev.max() <= 4 * twin.max() + 1e-7, (dev.max(), twin.max())
    assert dev[big].max() <= 4 * twin[big].max() + 1e-7, (dev[big].max(), twin[big].max())      # ... and among the large regions alone
    assert np.abs(g["flux"][diff] - o["flux"][diff, 1]).max() < 1e-3
    sc.close()


def test_region_sum_tasks_at_two_sizes(built, monkeypatch):
    """k_flux_split / k_flux_tasks through a render of bidir_room (res 48, 2 spp) with WTGPU_FLUX_TASK_TRIS=128 and with the default (2048): the
    same films to rtol 1e-9 (the f64 atomic sums take another order), every counter equal, and with WTGPU_PROFILE=1 the task counter (scratch
    slot 0) > 0 in both runs and larger at 128.  Regions overflow the bounded list at this size as it is (the scene's default mesh_detail, 1;
    measured: 2 tasks at the default, 10 at 128), so neither res nor mesh_detail had to be raised."""
    from wave_tracer_amd import Scene, render
    monkeypatch.setenv("WTGPU_PROFILE", "1")
    films, counters, tasks = {}, {}, {}
    for setting in ("128", None):
        if setting is None:
            monkeypatch.delenv("WTGPU_FLUX_TASK_TRIS", raising=False)
        else:
            monkeypatch.setenv("WTGPU_FLUX_TASK_TRIS", setting)
        sc = Scene("bidir_room", res=48, lut=(32, 32))
        films[setting] = render(sc, 2, seed=19, device=0)
        counters[setting] = sc.counters()
        tasks[setting] = int(sc.profile_counters(8)[0])
        sc.close()
    print(f"region-sum tasks: {tasks}; counters {counters[None]}")
    assert tasks[None] > 0 and tasks["128"] > tasks[None], tasks
    assert counters["128"] == counters[None], (counters["128"], counters[None])
    for a, b in zip(films["128"], films[None]):
        assert np.allclose(a, b, rtol=1e-9, atol=1e-30)
