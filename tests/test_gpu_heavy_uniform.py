"""The wave-cooperative traversal with its wave-uniform state in scalar registers (wt/coop.h: uniform(); k_trace_heavy, k_query_regions).

uniform() takes the first lane's copy of a value; a value that is NOT the same in all lanes would come out wrong without any fault.  So:
  * region queries (wtgpu_query_regions -> k_query_regions: coop_traverse, coop_ray_query, coop_cone_any, coop_cone_query) at the smallest shapes
    that reach every branch of the cone query, against the CPU checker's brute-force scan of all triangles against the final slab and, for the
    ray-like and the missing cones, against a numpy / f64 loop over all triangles;
  * the records of k_trace_heavy itself: one small render on which walks are handed to the wavefront kernel — twice (the same films, bit for
    bit) and once with every walk kept in its lane (WTGPU_CONE_BUDGET at its maximum), within the tolerance the parity table holds for the scene.

wtgpu_query_regions reports a region by its triangle COUNT, the triangle under the axis and the sorted set of classified edges (not by triangle
ids): these are what is compared; the counts and the edge sets must be equal for every cone."""
import numpy as np
import pytest

import parity
from test_gpu_traversal import oracle_regions, region_cones
from test_oracle import _tris

pytestmark = pytest.mark.gpu


def _cones():
    """84 cones at the 14K-triangle stand-in meshes: 64 beams of every width (regions of 1 .. 168 triangles: single partial batches of the exact
    test below 64, several above), 8 very wide ones (regions of hundreds to > 1000 triangles), 8 ray-like ones (cone_is_ray), 4 that miss."""
    wide = region_cones(8, 23)
    wide[:, 6] = np.linspace(.25, .5, 8)
    ray = region_cones(8, 24)
    ray[:, 6:8] = 0
    miss = region_cones(4, 25)
    miss[:, :3] = [1., 1., 1.]
    miss[:, 3:6] = [1., 0., 0.]
    return np.concatenate([region_cones(64, 22), wide, ray, miss]).astype(np.float32)


@pytest.fixture(scope="module")
def regions(built):
    from wave_tracer_amd import Scene
    sc = Scene("cornell_box", res=16, mesh_detail=0, lut=(32, 32))
    sc.upload(0)
    cones = _cones()
    out = sc, cones, sc.query_regions(cones), oracle_regions(sc, cones)
    yield out
    sc.close()


def test_region_queries_reach_every_branch(regions):
    """The cases themselves, from the checker's brute-force counts: a partial batch, several batches, far beyond the 64-triangle list, rays, misses."""
    sc, cones, g, o = regions
    n, diff = o["ntris"][:, 1], (o["flags"] & 3) == 0
    assert (diff & (n > 0) & (n < 64)).sum() >= 16 and (diff & (n >= 65) & (n <= 200)).sum() >= 1 and (diff & (n > 200)).sum() >= 3 and n.max() > 1000
    assert ((o["flags"][72:80] & 2) != 0).all() and (o["flags"][80:] == 1).all()
    assert (diff & (o["nedges"][:, 1] > 0)).sum() > 20
    assert (o["ntris"][diff, 0] == o["ntris"][diff, 1]).all() and (o["edges_list"] == o["edges_slab"]).all()   # the checker's record == its brute force


def test_region_queries_equal_brute_force(regions):
    """Closest distance (1e-5 relative, the tolerance of test_whole_region_queries_beyond_the_list_cap), flags (empty / ballistic / front face), the
    triangle under the axis, the region's triangle count and its sorted classified-edge set: equal for every cone."""
    sc, cones, g, o = regions
    fin = np.isfinite(o["dist"])
    diff = (o["flags"] & 3) == 0
    print("dist max rel", np.abs(g["dist"][fin] / o["dist"][fin] - 1).max(), "count differs at", np.nonzero(g["ntris"][diff] != o["ntris"][diff, 1])[0],
          "primary differs at", np.nonzero(g["primary"] != o["primary"])[0])
    assert (g["flags"] == o["flags"]).all()
    assert (np.isfinite(g["dist"]) == fin).all() and np.allclose(g["dist"][fin], o["dist"][fin], rtol=1e-5, atol=1e-7)
    assert (g["primary"] == o["primary"]).all()
    assert (g["ntris"][diff] == o["ntris"][diff, 1]).all()
    assert (g["nedges"][diff] == o["nedges"][diff, 1]).all() and (g["edges"][diff] == o["edges_slab"][diff]).all()
    df = np.abs(g["flux"][diff] - o["flux"][diff, 1])
    assert df.max() < 1e-3 and np.percentile(df, 95) < 2e-5, (df.max(), np.percentile(df, 95))


def test_ray_like_and_missing_cones_against_f64_loop(regions):
    """cone_is_ray: the answer is the closest hit of the axis — a Moeller-Trumbore loop over all triangles in f64.  The four cones that point away
    from everything: no triangle in front of them."""
    sc, cones, g, o = regions
    T = _tris(sc).astype(np.float64)
    a, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    for i in range(72, 84):
        org, d = cones[i, :3].astype(np.float64), cones[i, 3:6].astype(np.float64)
        d /= np.linalg.norm(d)
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(1)
        ok = np.abs(det) > 1e-30
        inv = np.where(ok, 1 / np.where(ok, det, 1), 0)
        tv = org - a
        u = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        v = (qv * d).sum(1) * inv
        t = (e2 * qv).sum(1) * inv
        m = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        if i >= 80:
            assert not m.any() and g["flags"][i] == 1 and g["primary"][i] == 0xFFFFFFFF and g["ntris"][i] == 0
            continue
        assert m.any() and g["flags"][i] & 2 and not g["flags"][i] & 1
        tb, j = t[m].min(), int(g["primary"][i])
        assert abs(g["dist"][i] - tb) < 1e-5 * tb + 1e-7, (i, g["dist"][i], tb)
        assert m[j] and abs(t[j] - tb) < 1e-6                       # the reported triangle is (one of) the closest
        assert bool(g["flags"][i] & 4) == bool(np.dot(T[j, 3], d) < 0)


DENSE = dict(res=64, mesh_detail=1, lut=(128, 128), crop_of=1440)   # test_cornell_dense_mesh_parity's scene: 283K triangles, hand-overs


def _render(spp=1, seed=3, twice=False):
    from wave_tracer_amd import Scene, render, develop
    sc = Scene("cornell_box", **DENSE)
    films = [render(sc, spp, seed=seed, device=0) for _ in range(2 if twice else 1)]
    out = films, develop(sc, *films[0], spp).astype(np.float64), sc.counters(), sc.profile_counters(8)
    sc.close()
    return out


def test_heavy_records_identical_and_like_the_per_lane_form(built, monkeypatch):
    """64 x 64 x 1 spp of the bench geometry.  (1) With WTGPU_PROFILE=2 (k_trace_heavy_prof, the same body with its phase clocks) the kernel counts its
    items: walks ARE handed over on this scene.  (2) Two default renders in one process: the same films bit for bit.  (3) The largest WTGPU_CONE_BUDGET
    keeps every cone query in its lane (only a full per-lane stack still hands over): the developed image within the parity table's tolerance
    for this scene (cornell_dense_mesh_parity)."""
    films, img, ctr, _ = _render(twice=True)
    for x, y in zip(*films):
        assert np.array_equal(x, y)
    assert ctr["traversal_stack_dropped"] == 0
    monkeypatch.setenv("WTGPU_PROFILE", "2")
    films_p, img_p, ctr_p, prof = _render()
    print("heavy items", prof[4], "segments", ctr_p["segments"])
    assert prof[4] > 0
    for k in ("segments", "ray_queries", "cone_queries", "cone_tri_overflow"):   # (the counters the kernel sums wave-uniformly)
        assert ctr_p[k] == ctr[k] // 2, (k, ctr_p[k], ctr[k])
    monkeypatch.delenv("WTGPU_PROFILE")
    monkeypatch.setenv("WTGPU_CONE_BUDGET", str(0xFFFFFFFE))   # (0xFFFFFFFF is the checker's "unbudgeted": no hand-over of a full stack either)
    _, img_l, ctr_l, _ = _render()
    err = np.abs(img - img_l).sum() / np.abs(img_l).sum()
    print("default vs per-lane form: rel L1", err, "segments", ctr["segments"] // 2, ctr_l["segments"])
    assert err <= parity.tolerance("cornell_dense_mesh_parity", 2e-2), err
