"""profiles/heavy_3waves_kernel_resources.txt (tools/kernel_resources.sh: the code-object metadata of a gfx950 build, no GPU needed): the wave-per-walk
traversal kernel keeps no vector register in memory, and either fits three wavefronts per SIMD with the launch bound saying so, or the bound stayed 2."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse():
    rows, bound = {}, None
    for line in open(os.path.join(ROOT, "profiles", "heavy_3waves_kernel_resources.txt")):
        m = re.match(r"#\s*k_trace_heavy launch_bound (\d+)", line)
        if m:
            bound = int(m.group(1))
        m = re.match(r"(k_\w+)\s+vgpr\s+(\d+)\s+spill\s+(\d+)\s+sgpr_spill\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = dict(zip(("vgpr", "spill", "sgpr_spill", "lds", "scratch"), map(int, m.groups()[1:])))
    return rows, bound


def test_heavy_kernel_resources():
    rows, bound = _parse()
    assert len(rows) >= 40 and "k_query_regions" in rows, "the file no longer lists every kernel"
    k = rows["k_trace_heavy"]
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert bound in (2, 3), "the file must say which launch bound k_trace_heavy was built with"
    if bound == 3:
        assert k["vgpr"] <= 168 and k["lds"] <= 13653, k   # 512 registers per lane and SIMD / 3; 160 KiB of LDS / 12 blocks per CU


def test_the_file_states_the_bound_the_source_sets():
    _, bound = _parse()
    hdr = open(os.path.join(ROOT, "wave_tracer_amd", "csrc", "wtgpu_kernels.h")).read()
    assert int(re.search(r"#define WTGPU_LB_HEAVY (\d+)", hdr).group(1)) == bound
