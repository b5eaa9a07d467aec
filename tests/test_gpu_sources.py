"""The device's emitter / sensor / wavenumber layer query by query (wtgpu_test_source_queries, kernels_test.hip: k_test_sources; wt/sources_probe.h)
on the sets of tests/test_sources_probe.py: the device against the CPU checker word by word (bit for bit where no libm call is involved),
against the f64 restatement with the CPU test's bounds, the finiteness of every output, the tail of the last block, and the rejected queries."""
import numpy as np
import pytest

import sources_probe as sp
from test_sources_probe import TOL, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev_sets(built):
    from wave_tracer_amd import Scene
    out = []
    for name, sc, R, qs in sp.source_sets(Scene):
        sc.upload(0)
        out.append((name, sc, R, {kind: (q, sc.source_queries(q)) for kind, q in qs.items()}))
    return out


def _types(R, q, chk):
    """per query: the type of the emitter the op worked on (-1: none) and the sensor's"""
    et = np.full(len(q), -1)
    types = np.array([int(e["type"]) for e in R.emitters])
    for i in range(len(q)):
        name = sp.OPS[int(q[i, 0])]
        if name == "emit":
            et[i] = types[int(q[i, 1])]
        elif name == "emit_direct":
            et[i] = types[int(chk[i, sp.W_A])]
    return et, int(R.sensor["type"])


def test_device_against_checker(dev_sets):
    """Outside the rounding band of the f64 thresholds: the uniforms and every discrete word identical; every float word whose computation
    calls no libm function bit-identical (signed zeros included); the words behind sinf / cosf / acosf (sources_probe.libm_words) within
    2 x TOL of each other, relative to max(|checker|, 1e-3 of the field's largest entry), beyond the f64 conditioning spread."""
    n_bits = n_libm = 0
    for name, sc, R, qs in dev_sets:
        for kind, (q, dev) in qs.items():
            chk = sp.oracle_source_queries(sc, q)
            assert np.array_equal(dev[:, sp.W_U:sp.W_U + sp.NU], chk[:, sp.W_U:sp.W_U + sp.NU]), (name, kind)      # the same uniforms
            et, st = _types(R, q, chk)
            fd, fc = dev.view(np.float32).astype(np.float64), chk.view(np.float32).astype(np.float64)
            word_field = {w: f for f, ws in sp.FIELDS.items() for w in ws}
            fmax = {}
            worst, band = {}, 0
            for i in range(len(q)):
                opn = sp.OPS[int(q[i, 0])]
                u = chk[i, sp.W_U:sp.W_U + sp.NU].view(np.float32)
                ref, v0, spread, dec = sp.f64_with_bound(R, q[i], u)
                same_discrete = np.array_equal(dev[i, sp.DISCRETE_WORDS], chk[i, sp.DISCRETE_WORDS])
                if dec.band and not same_discrete:        # the two f32 evaluations took different admissible branches
                    band += 1
                    continue
                assert same_discrete, (name, kind, i, opn, dev[i, sp.DISCRETE_WORDS], chk[i, sp.DISCRETE_WORDS])
                libm = set(sp.libm_words(opn, int(et[i]), st))
                exact = [w for w in sp.FLOAT_WORDS if w not in libm]
                if opn == "sense_direct" and fc[i, sp.W_BEAM + sp.B_SCALE] == 0:      # (no importance: the film offset may be a NaN of either sign)
                    exact = [w for w in exact if w not in sp.FIELDS["elem.offset"]]
                diff = [w for w in exact if dev[i, w] != chk[i, w]]
                assert not diff, (name, kind, i, opn, diff, fd[i, diff], fc[i, diff])
                n_bits += len(exact)
                for w in sorted(libm):
                    n_libm += 1
                    fld = word_field.get(w)
                    key = (opn, fld or "beam.frame")
                    if key not in fmax:
                        m = q[:, 0] == q[i, 0]
                        ws = sp.FIELDS.get(fld, [w])
                        vals = np.abs(fc[m][:, ws])
                        fmax[key] = float(vals[np.isfinite(vals)].max()) if np.isfinite(vals).any() else 0.0
                    sprd = (spread[w] + ref.get("extra_spread", {}).get(fld, 0.0)) if fld else 0.0
                    # (envelope x and frame: unit vectors)
                    floor = max(abs(fc[i, w]), 1e-3 * fmax[key], 1e-300) if fld else 1.0
                    e = max(abs(fd[i, w] - fc[i, w]) - 2 * sprd, 0.0) / floor
                    worst[key] = max(worst.get(key, 0.0), e)
                    bound = 2 * TOL.get((opn, fld), TOL["default"]) if fld else 2 * TOL.get((opn, "beam.d"), TOL["default"])
                    assert e <= bound, (name, kind, i, opn, w, key, e, bound, fd[i, w], fc[i, w])
            report("device vs checker", name, kind, len(q), band, {}, worst)
            if kind == "random":
                assert band <= len(q) // 100
    print(f"device vs checker: {n_bits} float words compared bit for bit, {n_libm} behind a libm call within 2 x TOL")
    assert n_bits > 500000


def test_device_against_f64(dev_sets):
    """the device against the f64 restatement with the CPU test's TOL and band rule"""
    for name, sc, R, qs in dev_sets:
        for kind, (q, dev) in qs.items():
            worst, band, fails, counts = sp.compare_f64(R, q, dev, TOL, kind)
            report("device vs f64", name, kind, len(q), band, counts, worst)
            assert not fails, (name, kind, len(fails), fails[:5])
            if kind == "random":
                assert band <= len(q) // 100, (name, band)
            fails = sp.check_properties(R, q, dev)
            assert not fails, (name, kind, len(fails), fails[:5])
            back, src = sp.sense_roundtrip_queries(R, q, dev)
            tol, fails = sp.roundtrip_failures(R, q, dev, back, sc.source_queries(back), src)
            assert not fails, (name, kind, len(fails), fails[:5])
            assert not sp.spot_cutoff_rows(R, q, dev)[2], (name, kind)
            assert not sp.film_border_rows(R, q, dev)[1], (name, kind)


def test_device_outputs_finite(dev_sets):
    """every float word of every query is finite on the device (or the -inf apex of a ray)"""
    for name, sc, R, qs in dev_sets:
        for kind, (q, dev) in qs.items():
            bad = sp.nonfinite_rows(q, dev)
            assert not len(bad), (name, kind, bad[:10])


def test_tail_of_the_last_block(dev_sets):
    """launches of 1, 63, 64, 65 queries and of the full set write the same rows (and nothing past the last one: the api allocates n rows)"""
    name, sc, R, qs = dev_sets[0]
    q, full = qs["random"]
    for n in (1, 63, 64, 65):
        assert np.array_equal(sc.source_queries(q[:n]), full[:n]), n
    assert np.array_equal(sc.source_queries(q), full)


def test_invalid_queries_are_rejected(dev_sets):
    """an op outside the table and an emitter index or tuid out of range return WTGPU_ERR_INVALID and launch nothing"""
    name, sc, R, qs = dev_sets[0]
    bad_op = sp.make_query("spectrum")
    bad_op[0] = len(sp.OPS)
    good = qs["random"][0][:3]
    for bad in (bad_op, sp.make_query("emit", i0=R.n_emitters), sp.make_query("kdist", i0=R.n_emitters), sp.make_query("Li", i0=0, i1=R.n_tris)):
        with pytest.raises(Exception, match="wtgpu error 1.*out of range"):
            sc.source_queries(np.concatenate([good, bad[None]]))
    assert np.array_equal(sc.source_queries(good), qs["random"][1][:3])      # the scene still answers
