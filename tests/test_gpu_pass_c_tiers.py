"""Pass C in tiers (WTGPU_PASS_C_TIERS=1: k_interact_c_prep — eight lanes per walk: intercepted power, tries 0-7 —, k_interact_c_wide and
k_interact_c_hard_tries — the tries that are left —, k_interact_c_commit — lane = walk) against the one-wavefront-per-walk form (k_interact_c /
k_interact_c_hard, WTGPU_PASS_C_TIERS=0) on the same scene, seed and samples.

Per walk both forms find the same accepted try (a try's draws depend on its index only, the lowest accepted try wins), the same recp_I (the same
f64 sum in the same tree: test_flux_tree_of_the_groups_equals_the_wave_butterfly, CPU) and call bdpt_walk_step<2> with the same arguments, so
  * EVERY counter is equal as an integer, between the forms and between the settings of the wide/hard boundary (WTGPU_PASS_C_EASY_TRIES = 8, 64, 512:
    every unsettled walk goes to the hard kernel / the default region / the wide kernel keeps nearly all of them);
  * the films get the same addends through f64 atomics in another order (the order of the next round's queue differs).
A round with few walks per wavefront of its grid runs one wavefront per walk inside k_interact_c_prep (WTGPU_PASS_C_THIN, default 8): every round of
scenes this small.  The boundary runs therefore set WTGPU_PASS_C_THIN=0 — groups of eight always — and one more run per case ("thin") keeps the
default; it must give the same counters, films and tier counts.

Tolerances: every film is compared as rel L1 = sum |a - b| / sum |b| against 10 x max(the spread MEASURED between two runs of the old form, floor);
spreads in tests/golden/pass_c_tiers_measured.json, recorded on the MI355X with PASS_C_TIERS_RECORD=<file to write them to>; a label the table does
not hold counts as a spread of 0.  The floors and their reasoning are those of test_gpu_connect_class.py — only the summation order may differ:
  * light, weight: 1e-14 — f64 sums of up to ~100 addends per pixel in another order: 100 x 2^-53 per pixel;
  * value: 1e-10 — the f32 rounding of a sample's f64 sum flips only where the sum lies within ~1e-15 of a rounding boundary; ONE walk that takes
    another try moves the film by > 1e-6.
The cases: the double slits at a small film; a dense cornell box (region-marker walks, whose power comes from k_flux_tasks' accumulator, next to
listed regions); the Fraunhofer furnace of test_gpu_render.py; one stream with batches that are no multiple of 64."""
import contextlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLE = os.path.join(ROOT, "tests", "golden", "pass_c_tiers_measured.json")
FACTOR = 10.0
FLOOR = {"value": 1e-10, "weight": 1e-14, "light": 1e-14}
BOUNDARIES = (8, 64, 512)

# name -> (scene, scene arguments, spp, samples per batch (0: the default), streams (0: the default))
CASES = {
    "double_slits96": ("double_slits", dict(res=96, lut=(64, 64)), 2, 0, 0),
    "cornell48_dense": ("cornell_box", dict(res=48, mesh_detail=1), 2, 0, 0),
    "furnace_fsd16": ("furnace", dict(res=16, fsd=1, lut=(128, 128)), 4, 0, 0),
    "double_slits96_batch1000": ("double_slits", dict(res=96, lut=(64, 64)), 2, 1000, 1),   # 1000, 1000, 304 | ...: no multiple of 64
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


_bases = {}


def _render(case, tiers, boundary=512, thin=0):
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import alloc_films
    name, kw, spp, batch, streams = CASES[case]
    if case not in _bases:   # the scene is baked once per case (the dense mesh takes seconds); every render uploads a handle of its own onto it
        _bases[case] = Scene(name, **kw)
    base = _bases[case]
    with _env(WTGPU_PASS_C_TIERS=tiers, WTGPU_PASS_C_EASY_TRIES=boundary, WTGPU_PASS_C_THIN=thin, **({"WTGPU_STREAMS": streams} if streams else {})):
        sc = Scene.from_desc(base.host_desc(), keepalive=base, name=name)   # (the knobs are read at upload)
        sc.upload(0, batch)
        dev = torch.device("cuda", 0)
        films = alloc_films(sc, dev)
        sc.reset_counters()
        sc.render_into(*films, 0, spp, 31, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        out = {"films": dict(zip(("value", "weight", "light"), (f.cpu().numpy().astype(np.float64) for f in films))), "counters": sc.counters(),
               "tiers": sc.pass_c_tiers()}
        sc.close()
    return out


_results = {}


def _case(case):
    """Two runs of the old form, one of the tiered form per boundary setting (groups of eight in every round) and one with thin rounds, once per module."""
    if case not in _results:
        r = {"old": _render(case, 0), "old2": _render(case, 0)}
        for b in BOUNDARIES:
            r[b] = _render(case, 1, b)
        r["thin"] = _render(case, 1, 512, thin=8)
        _results[case] = r
    return _results[case]


def _rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(1e-300, np.abs(b).sum()))


def _check(label, what, measured, spread, floor):
    """measured <= 10 x max(the committed old-vs-old spread of `label`, floor); PASS_C_TIERS_RECORD=<file> records `spread` there instead of reading the table."""
    out = os.environ.get("PASS_C_TIERS_RECORD")
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
    print(f"{label} [{what}]: tiers vs old form {measured:.3e}; old form twice {spread:.3e} (committed {committed:.3e}); tolerance {tol:.1e}")
    assert measured <= tol, f"{label} [{what}]: measured {measured:.3e}, tolerance {tol:.1e} = 10 x max(committed spread {committed:.3e}, floor {floor:.0e})"


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_counters_equal_as_integers(built, case):
    r = _case(case)
    old = r["old"]["counters"]
    print(case, {k: old[k] for k in ("fsd_interactions", "null_interactions", "vertices", "segments")})
    assert old == r["old2"]["counters"], (case, old, r["old2"]["counters"])
    for b in BOUNDARIES + ("thin",):
        new = r[b]["counters"]
        for k in old:
            assert isinstance(new[k], int) and new[k] == old[k], (case, b, k, old[k], new[k])
        assert new == old, (case, b, new, old)


@pytest.mark.gpu
def test_the_cases_hold_fraunhofer_interactions(built):
    n = {case: _case(case)["old"]["counters"]["fsd_interactions"] for case in CASES}
    print(n)
    assert sum(1 for v in n.values() if v > 100) >= 2, n


@pytest.mark.gpu
def test_every_tier_settles_walks_and_the_queues_have_ragged_ends(built):
    settled = {"prep": 0, "wide": 0, "hard": 0}
    ragged = short = 0
    for case in CASES:
        r = _case(case)
        assert all(v == 0 for k, v in r["old"]["tiers"].items() if k != "queue_lengths"), (case, r["old"]["tiers"])   # (the old form keeps none of this)
        # thin rounds count what the groups would have settled as theirs (the queue lengths: sorted, three streams record them in any order)
        assert {k: sorted(v) if k == "queue_lengths" else v for k, v in r["thin"]["tiers"].items()} == \
               {k: sorted(v) if k == "queue_lengths" else v for k, v in r[512]["tiers"].items()}, (case, r["thin"]["tiers"], r[512]["tiers"])
        for b in BOUNDARIES:
            t = r[b]["tiers"]
            print(case, "boundary", b, t)
            assert t["prep"] + t["wide"] + t["hard"] == t["walks"] > 0, (case, b, t)   # every pass-C walk is settled by exactly one tier
            assert t["walks"] == r[BOUNDARIES[0]]["tiers"]["walks"], (case, b)
            assert t["prep"] == r[BOUNDARIES[0]]["tiers"]["prep"], (case, b)            # (prep does not know the boundary)
            if b == 8:
                assert t["wide"] == 0, (case, t)                                         # the wide kernel has no try of its own: all of them go on
            for k in settled:
                settled[k] += t[k]
            # the device's own census of the rounds, and the same read off the queue lengths it kept (the first 56 rounds with a queue)
            q = np.asarray(t["queue_lengths"], dtype=np.int64)
            assert (q > 0).all() and q.size == min(t["rounds"], 56)
            if t["rounds"] <= 56:
                assert q.sum() == t["walks"] and (q % 8 != 0).sum() == t["rounds_not_multiple_of_8"] and (q < 8).sum() == t["rounds_shorter_than_8"]
            ragged += t["rounds_not_multiple_of_8"]
            short += t["rounds_shorter_than_8"]
    print("settled", settled, "rounds with a queue that is no multiple of 8:", ragged, "shorter than 8:", short)
    assert settled["prep"] > 0 and settled["wide"] > 0 and settled["hard"] > 0, settled
    assert ragged > 0 and short > 0, (ragged, short)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("film", ["value", "weight", "light"])
def test_films_differ_by_summation_order_only(built, case, film):
    r = _case(case)
    b0, b2 = r["old"]["films"][film], r["old2"]["films"][film]
    for b in BOUNDARIES + ("thin",):
        a = r[b]["films"][film]
        assert np.isfinite(a).all()
        if not b0.any():   # (a scene whose strategies leave this film empty)
            assert not a.any() and not b2.any()
            continue
        _check(f"{case}_{film}", f"boundary {b}", _rel_l1(a, b0), _rel_l1(b2, b0), FLOOR[film])


_PARENT = os.path.join(ROOT, "tests", "golden", "pass_c_counters_parent.json")
_ORDER_FREE_TIERS = ("walks", "prep", "rounds", "rounds_not_multiple_of_8", "rounds_shorter_than_8")   # (neither the boundary nor the streams' order move these)


def _tiers_pinned(t, every_tier):
    """The tier counts that a rerun must reproduce: `every_tier` adds wide / hard, which hold at the fixture's boundary (512) only; the queue
    lengths sorted, and only while every round's length was kept (beyond 56 rounds the streams' order decides which ones are)."""
    out = {k: int(t[k]) for k in _ORDER_FREE_TIERS + (("wide", "hard") if every_tier else ())}
    if t["rounds"] <= 56:
        out["queue_lengths"] = sorted(int(v) for v in t["queue_lengths"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_counters_equal_those_of_the_parent_commit(built, case):
    """Both forms share their device functions (pass_c_tries, pass_c_commit_walk, ...), so their agreement no longer says that either is right:
    tests/golden/pass_c_counters_parent.json holds, per case, counters() of the old form and pass_c_tiers() at boundary 512 as the kernels of
    commit 366ab4f (before the pieces were shared) gave them on the MI355X, seed 31; PASS_C_PARENT_RECORD=<file> writes such a table.  Every run
    of the module — old form twice, boundaries 8 / 64 / 512, thin rounds — gives those integers."""
    r = _case(case)
    out = os.environ.get("PASS_C_PARENT_RECORD")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        try:
            with open(out) as f:
                rec = json.load(f)
        except (OSError, ValueError):
            rec = {}
        rec[case] = {"counters": {k: int(v) for k, v in r["old"]["counters"].items()},
                     "tiers": {k: [int(x) for x in v] if k == "queue_lengths" else int(v) for k, v in r[512]["tiers"].items()}}
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        parent = rec[case]
    else:
        with open(_PARENT) as f:
            parent = json.load(f)[case]
    assert parent["tiers"]["walks"] > 0, (case, parent)
    for run in ("old", "old2") + BOUNDARIES + ("thin",):
        new = r[run]["counters"]
        assert set(new) == set(parent["counters"]), (case, run, sorted(new), sorted(parent["counters"]))
        for k, v in parent["counters"].items():
            assert isinstance(new[k], int) and new[k] == v, (case, run, k, v, new[k])
    for run in BOUNDARIES + ("thin",):
        every_tier = run in (512, "thin")
        assert _tiers_pinned(r[run]["tiers"], every_tier) == _tiers_pinned(parent["tiers"], every_tier), (case, run, r[run]["tiers"], parent["tiers"])


def _butterfly(v, offsets):
    """`flux += __shfl_xor(flux, off)` over the last axis, for every offset in turn: every lane adds its partner's value to its own."""
    lanes = np.arange(v.shape[-1])
    for off in offsets:
        v = v + v[..., lanes ^ off]
    return v


@pytest.mark.parametrize("n", [1, 7, 8, 9, 33, 64])
def test_flux_tree_of_the_groups_equals_the_wave_butterfly(n):
    """CPU, numpy f64: lane j of 64 holds triangle j (zero beyond the list) and the wavefront reduces by xor 32 .. 1 (pass_c_region_power_wave); group lane
    s of 8 holds t_k = triangle s + 8 k, adds ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7)) and the group reduces by xor 4, 2, 1
    (k_interact_c_prep).  The same tree: equal bit for bit, in every lane."""
    rng = np.random.default_rng(1000 + n)
    # non-negative fluxes over many orders of magnitude (a sum of equal-sized terms would round the same way in most trees)
    v = np.zeros((1000, 64))
    v[:, :n] = rng.random((1000, n)) * 10.0 ** rng.integers(-12, 1, (1000, n))
    wave = _butterfly(v, (32, 16, 8, 4, 2, 1))
    assert (wave == wave[:, :1]).all()   # every lane ends with the same bits
    t = v.reshape(1000, 8, 8)            # [draw][k][s]: triangle s + 8 k
    lane = ((t[:, 0] + t[:, 4]) + (t[:, 2] + t[:, 6])) + ((t[:, 1] + t[:, 5]) + (t[:, 3] + t[:, 7]))
    group = _butterfly(lane, (4, 2, 1))
    assert group.shape == (1000, 8)
    assert np.array_equal(group.view(np.uint64), wave[:, :8].view(np.uint64))
    # (and the tree matters: the plain left-to-right sum differs in some draws once there are enough terms)
    if n >= 9:
        assert (np.cumsum(v, axis=1)[:, -1] != wave[:, 0]).any()
