"""The device's material layer query by query (wtgpu_test_bsdf_queries, kernels_test.hip: k_test_bsdf; wt/bsdf_probe.h): the class forms of the
material-sorted interaction pass against the generic form, the device against the CPU checker and against the f64 restatement
(tests/bsdf_probe.py), the finiteness of every output; a small render of a rough surface_spm ground at 10 GHz.  Then pass A's forms
(WTGPU_SORTED_INTERACT x WTGPU_COOP_IO x WTGPU_LIGHT_ROUNDS) render the same."""

import numpy as np
import pytest

import bsdf_probe as bp
import parity
from test_bsdf_probe import TOL

pytestmark = pytest.mark.gpu

FLOATS = ("f", "pdf", "wo", "dpd", "eta", "M", "pdf_rev")


@pytest.fixture(scope="module")
def dev_sets(built):
    from wave_tracer_amd import Scene
    sets = bp.bsdf_sets(Scene, np.random.default_rng(11))
    out = []
    for label, sc, q, meta in sets:
        sc.upload(0)
        gen = sc.bsdf_queries(q, -1)
        out.append((label, sc, q, gen))
    return out


def test_class_forms_bit_identical_to_generic(dev_sets):
    """material_pdf<CLS> / material_sample<CLS> (the class kernels of WTGPU_SORTED_INTERACT=1, 2) write every output word bit-identical to the
    generic form, signed zeros included, on every query of an unwrapped material of that class; elsewhere they report `not applicable`."""
    n_cls = 0
    for label, sc, q, gen in dev_sets:
        types = np.array([int(bp.material_record(sc, int(m))["type"]) for m in range(sc.info.n_materials)])
        assert (gen[:, 0] & 1).all()
        for cls in (bp.MAT_DIFFUSE, bp.MAT_DIELECTRIC, bp.MAT_SURFACE_SPM):
            out = sc.bsdf_queries(q, cls)
            mine = types[q[:, 0]] == cls
            assert ((out[:, 0] & 1) != 0).tolist() == mine.tolist(), (label, cls)
            assert not out[~mine].any(), (label, cls)
            diff = np.flatnonzero((out[mine] != gen[mine]).any(axis=1))
            assert diff.size == 0, (label, cls, diff[:5], out[mine][diff[:1]], gen[mine][diff[:1]])
            n_cls += int(mine.sum())
    assert n_cls >= 10000
    print(f"class forms: {n_cls} queries bit-identical to the generic form")


def _f64_info(sc, q, d):
    """per query: in the rounding band of a decision, the f64 conditioning spread [41], the (1 - alpha) rounding terms"""
    fms, info = {}, []
    for i in range(len(q)):
        fm = fms.setdefault(int(q[i, 0]), bp.F64Material(sc, int(q[i, 0])))
        ref, _, spread = bp.f64_with_bound(fm, q[i], d["u"][i])
        info.append((bp.in_band(ref, d["u"][i]), spread, ref["cond"]))
    return info


def test_device_against_checker(dev_sets):
    """The device's generic form against the checker's (oracle_bsdf_queries), query by query: the uniforms, valid, specular / scattered,
    reflection / transmission and the draws consumed identical outside the rounding band of the f64 thresholds (counted and printed); the
    floats per field within parity.check's label bsdf_queries/<field>: the error beyond 32 x the f64 conditioning spread and the (1 - alpha)
    rounding, relative to max(|checker|, 1e-3 of the field's largest entry), for f and M relative to the matrix's largest entry.  Grazing
    directions included: both sides run the same f32 arithmetic (-ffp-contract=off), only libm differs."""
    worst = {k: 0.0 for k in FLOATS}
    n = nb = 0
    for label, sc, q, gen in dev_sets:
        out = bp.oracle_bsdf_queries(sc, q)
        g, o = bp.decode(gen), bp.decode(out)
        assert np.array_equal(gen[:, 41:47], out[:, 41:47]), label                  # the same uniforms
        same = (g["valid"] == o["valid"]) & (np.signbit(g["dpd"]) == np.signbit(o["dpd"])) & (g["draws"] == o["draws"]) & \
            (np.signbit(g["wo"][:, 2] * q[:, 3].view(np.float32)) == np.signbit(o["wo"][:, 2] * q[:, 3].view(np.float32)))
        info = _f64_info(sc, q, o)
        band = np.array([x[0] for x in info])
        assert (same | band).all(), (label, np.flatnonzero(~(same | band))[:10])
        nb += int((~same).sum())
        for i in np.flatnonzero(same & ~band):
            _, spread, cond = info[i]
            for key, sl in bp.FIELDS.items():
                if key not in ("f", "pdf") and not o["valid"][i]:
                    continue
                a = np.atleast_1d(g[key][i]).astype(np.float64)
                b = np.atleast_1d(o[key][i]).astype(np.float64)
                if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(spread[sl]).all()):
                    continue
                c = cond["f" if key == "f" else ("r" if key == "pdf_rev" else "p")]
                sc_ = max(np.abs(b).max(), 1e-30)
                floor = sc_ if key in ("f", "M") else 1e-3 * sc_
                e = np.maximum(np.abs(a - b) - 32 * spread[sl] - 16 * c * np.abs(b), 0) / np.maximum(np.abs(b), floor)
                worst[key] = max(worst[key], float(e.max()))
        n += len(q)
    for key in FLOATS:
        parity.check(f"bsdf_queries/{key}", worst[key], sanity=5e-2)
    print(f"device vs checker, {n} queries: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f"; discrete outcomes differing inside the "
          f"rounding band {nb}")


def test_device_against_f64(dev_sets):
    """The device's generic form against the f64 restatement with the bounds of tests/test_bsdf_probe.py (TOL beyond the conditioning spread;
    grazing directions, the (1 - alpha) cancellation and the gaussian sampler's logf as stated there)."""
    worst_all, band_all, thr_all, n = {}, 0, 0, 0
    for label, sc, q, gen in dev_sets:
        worst, band, fails, thr = bp.compare_f64(sc, q, gen, TOL)
        assert not fails, (label, len(fails), fails[:5])
        for key, e in worst.items():
            worst_all[key] = max(worst_all.get(key, 0.0), e)
        band_all += band
        thr_all += thr
        n += len(q)
    for kind in sorted({k for k, _ in worst_all}):
        print(f"device vs f64 [{kind}]: " + ", ".join(f"{f} {e:.1e}" for (k, f), e in sorted(worst_all.items()) if k == kind))
    print(f"device vs f64: {n} queries, {band_all} inside the rounding band, {thr_all} on IOR_has_transmission's threshold (compared under the "
          f"f32 code's interface decision)")


def test_device_outputs_finite(dev_sets):
    """Every output of every query finite on the device (M where dpd != 0: every caller discards a sample of density 0), the rough
    surface_spm at 60 / 10 GHz included."""
    for label, sc, q, gen in dev_sets:
        d = bp.decode(gen)
        for key in FLOATS:
            bad = ~np.isfinite(d[key].reshape(len(q), -1)).all(axis=1)
            if key == "M":
                bad &= d["dpd"] != 0
            assert not bad.any(), (label, key, np.flatnonzero(bad)[:10])


@pytest.mark.parametrize("ground", ["ground", "ground_gauss"])
def test_render_rough_ground_at_10ghz(built, ground):
    """tests/data/xml/bsdf_probe.xml: a sunlit rough surface_spm ground (fractal resp. gaussian, roughness-parametrised) at 10 GHz, where the
    profile normalisations need the conditioned form: the device's films are finite, carry light, and equal the checker's under the label
    bsdf_probe_10GHz/<ground>.  (One plane under a directional light: every film contribution comes through a connection, i.e. material_f;
    sampled directions leave the scene, so the conditioned samplers are covered by the per-query tests only.  At 10 GHz both profiles'
    PSDs reduce to ~1/pi, which is why the two films agree with the checker to the same number.)"""
    from wave_tracer_amd import Scene, render, develop
    from oracle_util import oracle_render
    sc = Scene.from_xml(bp.XML, defines={"ground": ground})
    spp = 4
    v, w, l = render(sc, spp, seed=21, device=0)
    gpu = develop(sc, v, w, l, spp)
    ov, ow, ol, _ = oracle_render(sc, 0, spp, 21)
    cpu = develop(sc, ov, ow, ol, spp)
    assert np.isfinite(gpu).all() and np.isfinite(cpu).all() and cpu.sum() > 0
    err = np.abs(gpu.astype(np.float64) - cpu).sum() / max(1e-30, np.abs(cpu).sum())
    parity.check(f"bsdf_probe_10GHz/{ground}", err)
    print(f"bsdf_probe.xml ({ground}, 10 GHz): rel L1 device vs checker {err:.2e}")


@pytest.mark.parametrize("name,kw,spp", [("cornell_box", dict(res=24, mesh_detail=0), 2), ("bidir_room", dict(res=24), 2), ("furnace_spm", dict(res=24), 2)])
def test_pass_a_forms_render_the_same(built, monkeypatch, name, kw, spp):
    """Pass A's forms with light rounds on and off (WTGPU_FIRST_ROUNDS=2: the rounds beyond the second run in k_light_rounds when
    WTGPU_LIGHT_ROUNDS=1): WTGPU_SORTED_INTERACT 0 / 1 / 2 x WTGPU_COOP_IO 0 / 1 (k_interact_coop) x WTGPU_LIGHT_ROUNDS 0 / 1 — every counter
    equal, the films equal at the tolerance of test_material_sorted_pass_and_staged_connections_render_the_same."""
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    out = {}
    for sorted_ in (0, 1, 2):
        for coop in (0, 1):
            for light in (0, 1):
                monkeypatch.setenv("WTGPU_FIRST_ROUNDS", "2")
                monkeypatch.setenv("WTGPU_SORTED_INTERACT", str(sorted_))
                monkeypatch.setenv("WTGPU_COOP_IO", str(coop))
                monkeypatch.setenv("WTGPU_LIGHT_ROUNDS", str(light))
                sc = Scene(name, **kw)
                sc.upload(0, 2048)
                dev = torch.device("cuda", 0)
                films = alloc_films(sc, dev)
                st = torch.cuda.current_stream(dev).cuda_stream
                sc.reset_counters()
                sc.render_into(*films, 0, spp, 37, st)
                torch.cuda.synchronize(dev)
                out[(sorted_, coop, light)] = ([f.cpu().numpy() for f in films], sc.counters())
                sc.close()
    ref, cref = out[(0, 0, 0)]
    assert cref["surface_interactions"] > 100
    for mode, (films, c) in out.items():
        assert c == cref, (name, mode, c, cref)
        for a, b in zip(films, ref):
            assert np.allclose(a, b, rtol=2e-6, atol=1e-12 * max(1.0, float(np.abs(b).max()))), (name, mode, float(np.abs(a - b).max()))
