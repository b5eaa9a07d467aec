#!/usr/bin/env python3
"""Times the line-of-sight maps of a coverage sensor (Scene.line_of_sight: which emitters every element sees) in both forms of the kernel
beside the ray probe (wtgpu_trace_rays) on the same number of rays.

  per_sample   k_los_sample, one lane per (element, sample)            (WTGPU_LOS_PER_SAMPLE=1; 32 samples)
  per_pair     k_los_pair, one lane per (element, emitter)             (WTGPU_LOS_PER_SAMPLE=0; 32 samples)
  centres      samples = 0: the elements' centres, k_los_pair in either form
  *_visible    the same asking for VISIBLE and the ids only: the kernels that keep no direction sums
  probe_*      the yardstick: wtgpu_trace_rays, a CLOSEST-hit query with one lane per ray, on H W S E rays built once on the device — from the
               elements' centres (exactly the line-of-sight rays of `centres`), or from S points per element jittered by torch (the same
               number and distribution as the 32-sample query's, not the same draws), each towards its emitter, range [0, dist].  It reads
               32 bytes per ray and writes 20; the maps form their rays in registers and write a few floats per element.

Scene: the bundled etoile at 720 x 540, every emitter.  Every call is timed between two device events; the calls are alternated after a
warm-up and the median of --reps (>= 15) is reported, with the quotients over the probe — reported, not judged.  Prints one JSON line; --out
also writes it to a file.  Needs a GPU.  Not part of bench.py."""
import argparse
import os

from film_bench_util import alternate, event_ms, finish, need_gpu

SAMPLES, SEED, RES = 32, 1, 720
ALL = dict(maps=("visible", "distance", "direction", "cos"), elem=("point", "nearest_distance"), ids=("n_visible", "nearest"))
VISIBLE = dict(maps=("visible",), elem=(), ids=("n_visible", "nearest"))


def _upload(per_sample):
    """An uploaded scene whose knobs were read with WTGPU_LOS_PER_SAMPLE = per_sample (the knobs are read once per upload)."""
    from wave_tracer_amd import Scene
    old = os.environ.get("WTGPU_LOS_PER_SAMPLE")
    os.environ["WTGPU_LOS_PER_SAMPLE"] = per_sample
    try:
        return Scene("etoile", res=RES, mesh_detail=1).upload(0, 65536)     # a small batch: nothing is rendered here
    finally:
        os.environ.pop("WTGPU_LOS_PER_SAMPLE") if old is None else os.environ.__setitem__("WTGPU_LOS_PER_SAMPLE", old)


def _probe(sc, points):
    """-> a call that traces a ray from every point [..., 3] to every emitter that is not an area emitter, and the share of rays that arrive."""
    import torch
    from wave_tracer_amd.api import _check, load_library
    dev = points.device
    rays = []
    for e in sc.emitter_summary():
        if e["type"] == "area":
            continue
        p = points.reshape(-1, 3)
        if e["type"] == "directional":
            d = torch.tensor(e["direction"], dtype=torch.float32, device=dev).expand_as(p)
            t = torch.full((len(p), 1), float("inf"), dtype=torch.float32, device=dev)
        else:
            v = torch.tensor(e["position"], dtype=torch.float32, device=dev) - p
            t = v.norm(dim=-1, keepdim=True)
            d = v / t
        rays.append(torch.cat([p, d, torch.zeros_like(t), t], dim=-1))
    rays = torch.cat(rays).contiguous()
    n = len(rays)
    dist, tuid, front = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    bary = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    lib = load_library()

    def call():
        _check(lib.wtgpu_trace_rays(sc._h, None, rays.data_ptr(), n, dist.data_ptr(), tuid.data_ptr(), bary.data_ptr(), front.data_ptr()))
    call()
    torch.cuda.synchronize(dev)
    return call, n, float(torch.isinf(dist).float().mean().item())


def _calls():
    """-> ({label: the call}, what the result says of the scene and of the probe's rays)"""
    import torch
    sc, other = _upload("1"), _upload("0")
    dev = torch.device("cuda", 0)
    centres = sc.line_of_sight(0, SEED, maps=(), elem=("point",), ids=())["point"]
    ext = (centres[0, 1] - centres[0, 0]).abs() + (centres[1, 0] - centres[0, 0]).abs()      # (an element's extent along x, y; the sensor is axis-aligned)
    g = torch.Generator(device=dev).manual_seed(SEED)
    jitter = (torch.rand((sc.height, sc.width, SAMPLES, 3), dtype=torch.float32, device=dev, generator=g) - 0.5) * ext
    probe_centres, n_centres, free_centres = _probe(sc, centres)
    probe_samples, n_samples, free_samples = _probe(sc, centres[:, :, None, :] + jitter)
    del jitter
    calls = {"per_sample": lambda: sc.line_of_sight(SAMPLES, SEED, **ALL),
             "per_pair": lambda: other.line_of_sight(SAMPLES, SEED, **ALL),
             "per_sample_visible": lambda: sc.line_of_sight(SAMPLES, SEED, **VISIBLE),
             "per_pair_visible": lambda: other.line_of_sight(SAMPLES, SEED, **VISIBLE),
             "probe_samples": probe_samples,
             "centres": lambda: sc.line_of_sight(0, SEED, **ALL),
             "centres_visible": lambda: sc.line_of_sight(0, SEED, **VISIBLE),
             "probe_centres": probe_centres}
    x, y = sc.line_of_sight(SAMPLES, SEED, **ALL), other.line_of_sight(SAMPLES, SEED, **ALL)
    assert all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in x), "the two forms differ"
    visible = float(x["visible"].mean().item())
    return calls, {"scene": "etoile", "film": [sc.width, sc.height], "triangles": int(sc.info.n_tris), "samples": SAMPLES,
                   "emitters": n_centres // (sc.width * sc.height), "rays": {"samples": n_samples, "centres": n_centres}, "mean_visible": visible,
                   "probe_rays_that_arrive": {"samples": free_samples, "centres": free_centres}}


def bench(reps):
    calls, about = _calls()
    med = alternate({k: (lambda fn=fn: event_ms(fn)[0]) for k, fn in calls.items()}, reps)
    over = {k: med[k] / med["probe_centres" if k.startswith("centres") else "probe_samples"] for k in med if not k.startswith("probe")}
    return dict(about, ms=med, over_probe=over,
                per_sample_over_per_pair={"all": med["per_sample"] / med["per_pair"], "visible": med["per_sample_visible"] / med["per_pair_visible"]})


def kernel_only(label, reps):
    """One of the calls alone, for `rocprofv3 --kernel-trace --stats -- python tools/bench_los.py --kernel-only LABEL`: the kernel's own time is
    the trace's average of its dispatches (the set-up dispatches one more of each line-of-sight kernel)."""
    import torch
    calls, _ = _calls()
    for _ in range(reps):
        calls[label]()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", default=None, metavar="LABEL", help="run this one call --reps times and print nothing (for a kernel trace)")
    args = ap.parse_args()
    need_gpu("bench_los")
    reps = max(15, args.reps)
    if args.kernel_only:
        return kernel_only(args.kernel_only, reps)
    finish(dict({"tool": "bench_los", "reps": reps}, **bench(reps)), args.out)


if __name__ == "__main__":
    main()
