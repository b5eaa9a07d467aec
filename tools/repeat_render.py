#!/usr/bin/env python3
"""Are two renders of one batch the same films, bit for bit?  N fresh scenes, two renders each; per pair the number of elements that differ in the
value, weight and light films.  WTGPU_LIB=<path> selects another build of the library (tools/build_variant.sh, or an older checkout's libwtgpu.so),
so that two builds can be compared run for run.  With the library of 24c3956 the value film of the default scene differed by one ulp in 1-4 elements
in 27 of 36 pairs on an MI355X (k_connect_splat_tiled added the tiles that meet in a film element in arrival order); since the ordered launches: 0.
usage: repeat_render.py [N] [scene] [res]        (default: 6 pairs of tests/test_gpu_heavy_uniform.py's scene)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wave_tracer_amd import Scene, render  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
name = sys.argv[2] if len(sys.argv) > 2 else "cornell_box"
kw = dict(res=int(sys.argv[3]), mesh_detail=0) if len(sys.argv) > 3 else dict(res=64, mesh_detail=1, lut=(128, 128), crop_of=1440)
bad = 0
for k in range(n):
    sc = Scene(name, **kw)
    a, b = [render(sc, 1, seed=3, device=0) for _ in range(2)]
    d = [int((np.asarray(x) != np.asarray(y)).sum()) for x, y in zip(a, b)]
    bad += any(d)
    print(k, "elements that differ (value, weight, light):", d, flush=True)
    sc.close()
print("pairs that differ:", bad, "of", n)
sys.exit(1 if bad else 0)
