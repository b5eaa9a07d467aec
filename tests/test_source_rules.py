"""Rules the device sources keep by hand, checked on the text (CPU suite).

Round 5's compiler finding (wtgpu_kernels.h: wave_grab0): a persistent loop of a one-wavefront block that BEGINS with
`if (threadIdx.x == 0) item = atomicAdd(head, 1)` can have that branch threaded with a branch on the same condition at the END of its body; the
63 other lanes then go round an inner loop of their own, for ever.  The rule: whatever lane 0 alone fetches for its wavefront goes through
wave_grab0 / wave_grab / wave_grab_item, or has a convergent operation (a barrier, a ballot, a shuffle) in the lines right in front of the branch.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wave_tracer_amd", "csrc")
LANE0_FETCH = re.compile(r"if \((?:threadIdx\.x(?: & 63u?)?|tid|lane)\s*==\s*(?:0u?|leader)\)\s*(?:\w+\s*=\s*)[^;]*(?:atomicAdd|_alloc)\(")
CONVERGENT = re.compile(r"__syncthreads\(\)|__ballot\(|__shfl|wave_barrier\(\)|wave_bcast0\(|wave_grab")


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "kernels_*.hip")) + [os.path.join(CSRC, "wtgpu_kernels.h")] + glob.glob(os.path.join(CSRC, "wt", "coop*.h")))


def test_lane0_fetches_sit_behind_a_convergent_operation():
    found, bad = 0, []
    for path in _sources():
        lines = open(path).read().split("\n")
        for i, l in enumerate(lines):
            if l.lstrip().startswith("//") or not LANE0_FETCH.search(l):
                continue
            found += 1
            before = "\n".join(x for x in lines[max(0, i - 6):i] if not x.lstrip().startswith("//"))
            if not CONVERGENT.search(before):
                bad.append(f"{os.path.relpath(path, ROOT)}:{i + 1}: {l.strip()}")
    assert found >= 4, "the pattern no longer matches the sources: update this test"
    assert not bad, "lane-0 fetch without a convergent operation in front of its branch:\n" + "\n".join(bad)


def test_one_wavefront_kernels_grab_through_the_helper():
    """No one-wavefront kernel hands its queue item through a __shared__ word any more (the 256-thread k_interact_c_hard does, between real barriers,
    the first of them in front of the branch)."""
    for path in _sources():
        src = open(path).read()
        for m in re.finditer(r"if \((?:threadIdx\.x|tid) == 0\) s_item = ", src):
            before = src[:m.start()].rstrip().split("\n")[-1]
            assert "__syncthreads();" in before, f"{os.path.relpath(path, ROOT)}: a shared queue word written without a barrier in front of the branch"
    hdr = open(os.path.join(CSRC, "wtgpu_kernels.h")).read()
    body = hdr[hdr.index("WT_D uint32_t wave_grab0("):]
    body = body[:body.index("}") + 1]
    assert body.index("wave_barrier()") < body.index("if (wave_first_lane())") < body.index("readfirstlane")


def _innermost_loops(asm_lines):
    """For every line of a function's assembly the header of the innermost loop its basic block belongs to (None outside loops), from the
    compiler's own block annotations."""
    out, loop, pending = [], None, None
    for l in asm_lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; %bb\.\d+:(.*)$", l)
        if m:
            label = m.group(1) if l.startswith(".L") else None
            comment = m.group(m.lastindex)
            loop, pending = None, label
            mm = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=\d+", comment)
            if mm:
                loop = mm.group(1)
            elif "Loop Header" in comment and label:
                loop = label[2:]
        elif pending is not None and re.match(r"^\s*;", l) and "; wave barrier" not in l:
            if "Loop Header" in l:
                loop = pending[2:]
        else:
            pending = None
        out.append(loop)
    return out


def test_minimal_reproducer_of_the_split_persistent_loop(tmp_path):
    """tools/repro_persistent_loop.hip, compiled for gfx950 here (no GPU needed): in k_new — the form of wave_grab0 — the marker, lane 0's atomic and
    the readfirstlane that hands the item over sit in ONE loop.  What the compiler makes of k_old, the idiom of rounds 2-5, is reported: with ROCm 7.2
    the atomic is in the outer of two loops and the load of the shared word in the header of the inner one — the hang of round 5."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import pytest
        pytest.skip("hipcc not found")
    asm = tmp_path / "repro.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "tools", "repro_persistent_loop.hip")],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read().split("\n")

    def body(name):
        a = next(i for i, l in enumerate(text) if l.startswith(name + ":"))
        b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
        return text[a:b]

    new = body("k_new")
    loops = _innermost_loops(new)
    at = [i for i, l in enumerate(new) if "global_atomic_add" in l]
    marks = [i for i, l in enumerate(new) if "; wave barrier" in l]
    assert len(at) == 1 and len(marks) >= 2
    opening = max(i for i in marks if i < at[0])
    closing = min(i for i in marks if i > at[0])
    reads = [i for i in range(at[0], closing + 12) if "v_readfirstlane_b32" in new[i]]
    assert reads, "no readfirstlane behind the atomic"
    involved = {loops[opening], loops[at[0]], loops[closing]} | {loops[i] for i in reads}
    assert len(involved) == 1 and None not in involved, f"k_new: the queue grab is spread over loops {involved}"
    old = body("k_old")
    lo = _innermost_loops(old)
    a0 = next(i for i, l in enumerate(old) if "global_atomic_add" in l)
    r0 = next(i for i, l in enumerate(old) if "ds_read_b32" in l)
    print(f"k_old with this compiler: atomic in loop {lo[a0]}, load of the shared item in loop {lo[r0]} -> " + ("SPLIT (the round-5 hang)" if lo[a0] != lo[r0] else "one loop"))


# ---- environment knobs -------------------------------------------------------------------------------------------------------------------------
# What is not a knob of the host driver and may still be put into an environment: the library / data locations and the two switches of the
# runtime-settings check (wtgpu_upload.hip); compile-time switches (-DWTGPU_...) are recognised by their use in the sources' #if lines.
NOT_KNOBS = {"WTGPU_LIB", "WTGPU_DATA_DIR", "WTGPU_ALLOW_SLOW_RUNTIME", "WTGPU_QUIET"}
ENV_USE = re.compile(r"""(?<!\w)(WTGPU_[A-Z0-9_]+)=(?!=)|["'](WTGPU_[A-Z0-9_]+)["']""")


def _knob_names():
    table = open(os.path.join(CSRC, "wtgpu_knobs.hip")).read()
    names = set(re.findall(r'^\s*\{"(WTGPU_[A-Z0-9_]+)", K\(', table, re.M))          # the table's records
    names |= set(re.findall(r'getenv\("(WTGPU_[A-Z0-9_]+)"\)', table))                 # the special cases beside it
    return names


def test_every_knob_a_tool_or_test_sets_is_in_the_knob_table():
    """A WTGPU_* name that tests/, tools/, bench.py or the Python package put into an environment is a name read_knobs reads (wtgpu_knobs.hip: the
    table and the special cases beside it), or one of the documented non-knobs: a tool that sets a knob nobody reads would measure nothing."""
    knobs = _knob_names()
    assert len(knobs) >= 40 and "WTGPU_GRID_CLS" in knobs and "WTGPU_STREAMS" in knobs, "the pattern no longer matches the knob table: update this test"
    compile_time = set()
    for path in glob.glob(os.path.join(CSRC, "**", "*.*"), recursive=True):
        if path.endswith((".hip", ".h", ".cpp", ".c")):
            for line in open(path, errors="replace"):
                if line.lstrip().startswith("#") and re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    compile_time |= set(re.findall(r"WTGPU_[A-Z0-9_]+", line))
    files = [os.path.join(ROOT, "bench.py")] + glob.glob(os.path.join(ROOT, "wave_tracer_amd", "*.py"))
    for d in ("tests", "tools"):
        for ext in ("py", "sh"):
            files += glob.glob(os.path.join(ROOT, d, "**", "*." + ext), recursive=True)
    used, unknown = set(), []
    for path in sorted(files):
        for i, line in enumerate(open(path, errors="replace")):
            for m in ENV_USE.finditer(line):
                name = m.group(1) or m.group(2)
                used.add(name)
                if name not in knobs and name not in NOT_KNOBS and name not in compile_time:
                    unknown.append(f"{os.path.relpath(path, ROOT)}:{i + 1}: {name}")
    assert len(used & knobs) >= 10, "the pattern no longer finds the knobs the tests set: update this test"
    assert not unknown, "set into an environment, read by nothing:\n" + "\n".join(unknown)


# ---- the work-item vocabulary ---------------------------------------------------------------------------------------------------------------------
def test_the_work_item_vocabulary_is_written_once():
    """What turns a queue item into a sample is a helper of wtgpu_kernels.h (the section next to walk_ident / queue_walk), not a copy per kernel
    form: the sample id and the Fraunhofer pool aggregate each stand ONCE in the kernel sources, and the connection kernels look their bucket up
    through bucket_of."""
    text = {p: open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "kernels_*.hip")) + [os.path.join(CSRC, "wtgpu_kernels.h")])}
    assert len(text) >= 11, "the pattern no longer matches the sources: update this test"
    all_text = "\n".join(text.values())
    sample_ids = re.findall(r"\(\s*\(uint64_t\)\s*pix\s*<<\s*32\s*\)", all_text)
    assert len(sample_ids) == 1, f"the sample-id expression occurs {len(sample_ids)} times: use sample_id_of"
    # the slice's pool, however its six fields are spelled (through a.st.ctl or a local ctl); kernels_test.hip's pool of a test probe is another one
    pools = re.findall(r"fsd_pool_t\s*\w*\s*\{[^{};]*(?:fsd_hdr|fsd_edges|fsd_cap|CTL_FSD_COUNTER|CTL_FSD_ECOUNTER|fsd_ecap)[^{};]*\}", all_text)
    assert len(pools) == 1, f"the fsd_pool_t aggregate is built {len(pools)} times: use fsd_pool_of"
    assert re.search(r"fsd_pool_t\{a\.st\.fsd_hdr, a\.st\.fsd_edges, a\.st\.ctl \+ CTL_FSD_COUNTER, a\.st\.fsd_cap, a\.st\.ctl \+ CTL_FSD_ECOUNTER, a\.st\.fsd_ecap\}", pools[0])
    hdr = text[os.path.join(CSRC, "wtgpu_kernels.h")]
    assert "<< 32" in hdr[hdr.index("sample_id_of("):hdr.index("fsd_pool_of(")] and "fsd_pool_t{a.st.fsd_hdr" in hdr
    assert "while (hi - lo > 1)" not in text[os.path.join(CSRC, "kernels_connect.hip")], "a bucket lookup written out: use bucket_of"
    assert "while (hi - lo > 1)" in hdr
