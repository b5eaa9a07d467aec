"""The class form of the connections (k_connect_class, WTGPU_CONNECT_CLASS=1: a work item is a SAMPLE, bucketed by the lengths (nT, nS) of its subpaths,
all of its strategies run in a row by one lane) against the strategy form (k_connect_strat, WTGPU_CONNECT_CLASS=0: a work item is one strategy of a
sample), on the same scene, seed and samples.

Both forms call bdpt_strategy with the same arguments for the same (sample, s, t), so
  * the counters `connections`, `shadow_rays`, `light_splats` are EQUAL as integers (a strategy that is skipped or run twice moves them);
  * the light image gets the same f32 addends through f64 atomics in another order, the weight film likewise;
  * the value film gets, per sample, the f32 rounding of the f64 sum of the same fluxes — summed by atomics in arrival order (strategy form) or in the
    lane in (t, s) order (class form).

Tolerances: every film is compared as rel L1 = sum |a - b| / sum |b| against 10 x the spread MEASURED between two runs of the strategy form
(tests/golden/connect_class_measured.json, recorded on the MI355X with CONNECT_CLASS_RECORD=<file to write the spreads to>), as
tests/parity.py does, with a floor under the measurement where two runs can happen to agree bit for bit (the recorded spreads are 0 for the weight films, 1e-20 .. 5e-18
for the value films and 1e-18 .. 6e-17 for the light images, the class form measured 0, 9e-20 .. 5e-18 and 4e-18 .. 2e-16 against them: all below
the floors, which therefore set the tolerances; a label the table does not hold counts as a measured spread of 0):
  * light, weight: 1e-14 — f64 sums of up to ~100 identical addends per pixel in another order: 100 x 2^-53 per pixel;
  * value: 1e-10 — the two f64 sums of a sample differ by ~1e-15 relative, so their f32 roundings differ (by one ulp, 6e-8 of that sample) only where
    the sum lies that close to a rounding boundary: about one sample in 1e8.  1e-10 of the film allows one sample in 600 to flip; ONE strategy missing from
    ONE sample of the few thousand here moves the film by > 1e-6.
The cases: a small cornell film (most classes hold fewer than 64 samples: partial wavefronts), the max_depth = 32 furnace of test_gpu_render.py (open
classes — subpaths beyond 17 vertices — and classes of a single sample), batches that are no multiple of 64."""
import contextlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLE = os.path.join(ROOT, "tests", "golden", "connect_class_measured.json")
FACTOR = 10.0
FLOOR = {"value": 1e-10, "weight": 1e-14, "light": 1e-14}

# name -> (scene, scene arguments, spp, samples per batch (0: a pass), one batch on one stream — its items are read back)
CASES = {
    "cornell48": ("cornell_box", dict(res=48, mesh_detail=0), 2, 2 * 48 * 48, True),
    "furnace_depth32": ("furnace", dict(res=16, max_depth=32, rr=0), 8, 8 * 16 * 16, True),
    "cornell48_batch1000": ("cornell_box", dict(res=48, mesh_detail=0), 2, 1000, False),   # 1000, 1000, 304 | 1000, 1000, 304: no multiple of 64
}


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _render(case, form, items=False):
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    name, kw, spp, batch, _ = CASES[case]
    with _env(WTGPU_CONNECT_CLASS=form, WTGPU_STAGED_CONNECT=0, **({"WTGPU_STREAMS": 1} if items else {})):
        sc = Scene(name, **kw)
        sc.upload(0, batch)
        dev = torch.device("cuda", 0)
        films = alloc_films(sc, dev)
        sc.reset_counters()
        sc.render_into(*films, 0, spp, 31, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        out = {"films": dict(zip(("value", "weight", "light"), (f.cpu().numpy().astype(np.float64) for f in films))), "counters": sc.counters()}
        if items:
            out["items"] = sc.connect_class_items(0)
        sc.close()
    return out


_results = {}


def _case(case):
    """Two runs of the strategy form and one of the class form, once per module."""
    if case not in _results:
        _results[case] = {"old": _render(case, 0), "old2": _render(case, 0), "new": _render(case, 1, items=CASES[case][4])}
    return _results[case]


def _rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(1e-300, np.abs(b).sum()))


def _check(label, measured, spread, floor):
    """measured <= 10 x max(the committed old-vs-old spread of `label`, floor); CONNECT_CLASS_RECORD=<file> records `spread` there instead of reading the table."""
    out = os.environ.get("CONNECT_CLASS_RECORD")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        try:
            with open(out) as f:
                rec = json.load(f)
        except (OSError, ValueError):
            rec = {}
        rec[label] = max(spread, rec.get(label, 0.0))
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        committed = spread
    else:
        with open(_TABLE) as f:
            table = json.load(f)
        committed = float(table.get(label, 0.0))   # (a label without a recorded spread: the floor alone, the strictest reading)
    tol = FACTOR * max(committed, floor)
    print(f"{label}: class vs strategy form {measured:.3e}; strategy form twice {spread:.3e} (committed {committed:.3e}); tolerance {tol:.1e}")
    assert measured <= tol, f"{label}: measured {measured:.3e}, tolerance {tol:.1e} = 10 x max(committed spread {committed:.3e}, floor {floor:.0e})"


@pytest.mark.parametrize("case", list(CASES))
def test_counters_equal_as_integers(built, case):
    r = _case(case)
    old, new = r["old"]["counters"], r["new"]["counters"]
    print(case, {k: (old[k], new[k]) for k in ("connections", "shadow_rays", "light_splats")})
    assert old["connections"] > 1000 and old["shadow_rays"] > 100
    for k in ("connections", "shadow_rays", "light_splats"):
        assert isinstance(new[k], int) and new[k] == old[k] == r["old2"]["counters"][k], (case, k, old[k], new[k])
    assert new == old, (case, new, old)   # (and every other counter: the walks are the same)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("film", ["value", "weight", "light"])
def test_films_differ_by_summation_order_only(built, case, film):
    r = _case(case)
    a, b, b2 = r["new"]["films"][film], r["old"]["films"][film], r["old2"]["films"][film]
    assert np.isfinite(a).all()
    if not b.any():   # (a scene whose strategies leave this film empty)
        assert not a.any() and not b2.any()
        return
    _check(f"{case}_{film}", _rel_l1(a, b), _rel_l1(b2, b), FLOOR[film])


def test_host_key_order_is_a_permutation_by_descending_work(built):
    from wave_tracer_amd.api import connect_class_order
    keys, KEY_DIM = connect_class_order()
    keys = keys.astype(np.int64)
    assert keys.size == KEY_DIM * KEY_DIM and np.array_equal(np.sort(keys), np.arange(keys.size))   # every key of the grid, each listed once
    work = (keys // KEY_DIM) * (keys % KEY_DIM)
    assert (np.diff(work) <= 0).all() and work[0] == (KEY_DIM - 1) ** 2 and work[-1] == 0


@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][4]])
def test_items_in_kernel_order_hold_every_sample_once(built, case):
    """The flattened item space as the kernel's wavefronts walk it: classes in the host's order, each padded to whole wavefronts, every sample of the
    batch in exactly one class — the one of its subpath lengths, as far as the strategy form's counters can tell: a class (tk, sk) below the open
    row / column runs a fixed number of strategies, and the sum over the samples equals `connections` (test_counters_equal_as_integers)."""
    from wave_tracer_amd.api import connect_class_order
    name, kw, spp, batch, _ = CASES[case]
    prefix, count, keys, items = (x.astype(np.int64) for x in _case(case)["new"]["items"])
    nb = batch   # one batch holds the whole render
    host_keys, KEY_DIM = connect_class_order()
    assert np.array_equal(keys, host_keys)                                  # the device built the host's permutation
    assert prefix[0] == 0 and np.array_equal(np.diff(prefix), (count + 63) // 64 * 64) and prefix[-1] % 64 == 0
    assert count.sum() == nb and np.array_equal(np.sort(items), np.arange(nb))   # each sample exactly once
    tk, sk = keys // KEY_DIM, keys % KEY_DIM
    open_ = (tk == KEY_DIM - 1) | (sk == KEY_DIM - 1)
    used = count > 0
    print(case, "classes used", int(used.sum()), "of them with < 64 samples", int((used & (count < 64)).sum()), "with one sample", int((count == 1).sum()),
          "samples in open classes", int(count[open_].sum()), "padding lanes", int(prefix[-1] - nb))
    assert (used & (count % 64 != 0)).sum() >= 3                             # partial wavefronts
    if case == "furnace_depth32":
        assert count[open_].sum() > 0 and (count == 1).sum() > 0           # open buckets, classes with a single sample
    else:
        assert count[open_].sum() == 0 and (used & (count < 64)).sum() >= 3   # no subpath beyond 17 vertices; classes with fewer than 64 samples
