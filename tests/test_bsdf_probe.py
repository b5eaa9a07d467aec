"""The CPU checker's material layer, one query at a time, against the f64 restatement of the reference's formulas (tests/bsdf_probe.py,
oracle/indep/second_source.py): diffuse, dielectric, surface_spm with the Dirac / fractal / gaussian profiles and the composite, mask, scale and
two-sided wrappers, textured reflectances, masks, scales and roughnesses (uv at texel centres, texel edges and wrap seams), at 380 nm .. 10 GHz
and at the edges (grazing and zero wi.z, the critical angle, IOR 1, the transmission threshold, the roughness clamp, composite bin edges,
masks of opacity 0, 0.6 and 1).  The device's forms are held against the same reference and against these host results in
tests/test_gpu_bsdf.py."""
import math

import numpy as np
import pytest

import bsdf_probe as bp

# Bound per field: the error beyond 16 x the f64 result's conditioning spread (bsdf_probe.f64_with_bound), relative to max(|ref|, 1e-3 of the
# query's scale).  What remains is f32 arithmetic on well-conditioned inputs.
# The gaussian profile's sampled direction (and the dpd, M and reverse pdf that follow it) is the exception: the truncated Box-Muller map takes
# logf(x) of x = (1 - s) u + s -> 1 (gaussian.hpp:34-36, the reference's f32 arithmetic above kProfileSmallArg), whose relative rounding is
# 2^-24 / |log x|; measured up to 2.1e-3.
# The weighted bsdf M of a scattered sample near the mirror direction carries the conductor amplitudes' phase at a half vector within a few
# ulps of the normal: measured up to 3.0e-4 of its largest entry.
TOL = {"default": 2e-4, "M": 5e-4, **{("spm_gaussian", f): 5e-3 for f in ("wo", "dpd", "M", "pdf_rev")}}


def _scene(name, **kw):
    from wave_tracer_amd import Scene
    return Scene(name, **kw)


@pytest.fixture(scope="module")
def sets(built):
    from wave_tracer_amd import Scene
    return bp.bsdf_sets(Scene, np.random.default_rng(11))


def _report(label, worst, band, n):
    kinds = sorted({k for k, _ in worst})
    for kind in kinds:
        items = ", ".join(f"{f} {e:.1e}" for (k, f), e in sorted(worst.items()) if k == kind)
        print(f"{label} vs f64 [{kind}]: {items}")
    print(f"{label}: {n} queries, {band} inside the rounding band of a sampling decision")


def test_checker_material_layer_against_f64(sets):
    """Every query of every set: the checker's discrete sample outcomes (valid, specular / scattered, reflection / transmission, null lobe,
    composite bin, draws consumed) equal the f64 replay from the same uniforms, except where the deciding uniform lies within the rounding
    band of the f64 threshold (counted); f, pdf, the sampled wo, dpd, eta, M and the reverse pdf within TOL beyond the conditioning."""
    total = band_total = thr_total = 0
    all_worst = {}
    for label, sc, q, meta in sets:
        out = bp.oracle_bsdf_queries(sc, q)
        d = bp.decode(out)
        assert d["applies"].all()
        worst, band, fails, thr = bp.compare_f64(sc, q, out, TOL)
        assert not fails, (label, len(fails), fails[:5])
        for key, e in worst.items():
            all_worst[key] = max(all_worst.get(key, 0.0), e)
        total += len(q)
        band_total += band
        thr_total += thr
        if label.startswith("tex_"):
            assert len(np.unique(q[:, 9:11], axis=0)) >= 10, label      # texel centres, edges and wrap seams
    _report("checker", all_worst, band_total, total)
    print(f"checker: {thr_total} queries on IOR_has_transmission's threshold, compared under the f32 code's interface decision")
    assert total >= 8000 and thr_total >= 1000
    assert band_total <= total // 1000


def test_checker_outputs_finite_at_radio_wavelengths(sets):
    """Every output word of every query is finite (M where dpd != 0: the gaussian sampler's density is 0 at wi.z = 1e-4, where 1 - |wi.xy|^2
    rounds to 0, and bdpt_walk_step / bdpt_surface_step / the plt_path walk discard such samples) — in particular the rough surface_spm at 60 GHz and 10 GHz, where the reference's f32
    normalisations 1 / (1 - e^-x) and 1 / (1 - (1 + y)^-s) are 1 / 0 (wt/bsdf.h: kProfileSmallArg; DESIGN.md, deviations)."""
    n_radio_scatter = 0
    for label, sc, q, meta in sets:
        d = bp.decode(bp.oracle_bsdf_queries(sc, q))
        for key in ("f", "pdf", "wo", "dpd", "eta", "M", "pdf_rev"):
            bad = ~np.isfinite(d[key].reshape(len(q), -1)).all(axis=1)
            if key == "M":    # a sample of density 0 (every caller discards it: bs.dpd == 0) may carry M = x / 0
                bad &= d["dpd"] != 0
            assert not bad.any(), (label, key, np.flatnonzero(bad)[:10])
        k = q[:, 7].view(np.float32)
        radio = k < 2 * math.pi / 3.0
        n_radio_scatter += int((radio & d["valid"] & (d["dpd"] > 0)).sum())
    assert n_radio_scatter >= 100


def test_profile_normalisation_small_argument():
    """The conditioned normalisations against f64 across the threshold: below kProfileSmallArg the f32 form is within 1e-6 of f64 (measured
    1.3e-7), above it
    the reference's expression is kept (its error there is at most ~6e-8 / 1e-4 = 6e-4: the price of leaving every bundled scene bit-identical,
    the smallest bundled argument being double_slits' k^2 T = 3.1e-4)."""
    lib = bp.load_oracle()
    import ctypes as C
    lib.kat_fractal_psd.argtypes = [C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.kat_fractal_psd.restype = C.c_float
    wi = np.array([0, 0, 1], np.float32)
    leafs = []
    for lam in [550e-6, 5e-2, 1.0, 5.0, 29.9792458, 300.0]:
        k = bp.k_of(lam)
        for rough, gamma in [(0.3, 3.0), (0.05, 3.0), (0.3, 2.5), (0.1, 4.0)]:
            got = lib.kat_fractal_psd(rough, gamma, k, wi.ctypes.data, wi.ctypes.data)
            leaf = {"profile": "fractal", "roughness": float(np.float32(rough)), "gamma": gamma, "sigma": 0.0}
            ref = bp.ss.profile_psd_z(leaf, 0.0, 0.0, k)
            T = bp.ss.profile_params(leaf, k)[0]
            y = k * k * T
            e = abs(got - ref) / ref
            assert math.isfinite(got) and e < (1e-6 if y < 1e-4 else max(1e-5, 2e-7 / y)), (lam, rough, gamma, y, got, ref)
            leafs.append((lam, y, e))
    assert any(y < 1e-8 for _, y, _ in leafs)
