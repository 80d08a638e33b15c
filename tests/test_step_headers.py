"""The step kernel's headers (csrc/hip/step/*.h, rayprim.h, step_launch.h) are self-contained: a
translation unit that includes one of them alone compiles (hipcc -fsyntax-only, gfx950), with the default
switches and with the extended code and the per-env parameter reads compiled out.  The dispatcher
(step_dispatch.hip) includes none of step/, so it compiles no device code.  The three hand-kept tables of
the step kernel's parts name the same parts: build.py STEP_PARTS, the launch_part calls of launch_step
(step_dispatch.hip) and the single translation unit's explicit instantiations (step.hip).  No GPU needed."""
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIP = ROOT / "mujoco_ros2_simulation_amd" / "csrc" / "hip"
SWITCHES = [[], ["-DMRS_EXT=0", "-DMRS_PRM=0"]]


def _syntax_only(job):
    header, switches = job
    unit = f'#include "{header}"\n'
    return subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", *switches, "-x", "hip", "-"],
                          input=unit, capture_output=True, text=True)


def test_step_headers():
    assert '#include "step/' not in (HIP / "step_dispatch.hip").read_text()
    step_headers = sorted((HIP / "step").glob("*.h"))
    assert step_headers, "no headers under csrc/hip/step"
    headers = step_headers + [HIP / "rayprim.h", HIP / "step_launch.h"]
    assert all(h.exists() for h in headers)
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on the path")
    jobs = [(h, sw) for h in headers for sw in SWITCHES]
    with ThreadPoolExecutor(max_workers=16) as pool:
        results = list(pool.map(_syntax_only, jobs))
    failed = [f"{h.relative_to(HIP)} {' '.join(sw)}\n{r.stdout}{r.stderr}" for (h, sw), r in zip(jobs, results) if r.returncode != 0]
    assert not failed, "\n".join(failed)


SEL = {"kSelForward": 1, "kSelStep": 2, "kSelPrimal": 4, "kSelHelpers": 8, "kSelAll": 15, "kSelPlain": 3}


def _parts(text, pattern):
    """the (G, kernel set, ext, params, dyn) of every launch_part<...> that `pattern` finds in text"""
    out = []
    for args in re.findall(pattern, text):
        a = [x.strip() for x in args.split(",")]
        assert len(a) in (4, 5), args
        sel = 0
        for name in a[1].split("|"):
            sel |= SEL[name.strip()]
        flags = [{"true": 1, "false": 0}[x] for x in a[2:]] + [0] * (5 - len(a))  # (kDyn defaults to false)
        out.append((int(a[0]), sel, *flags))
    return out


def test_part_tables_agree():
    from mujoco_ros2_simulation_amd import build
    built = []
    for _, g, sel, ext, prm, dyn in build.STEP_PARTS:
        bits = 0
        for name in sel.split("|"):
            bits |= SEL[name.strip()]
        built.append((g, bits, ext, prm, dyn))
    assert len(set(built)) == len(built) == 16
    launched = _parts((HIP / "step_dispatch.hip").read_text(), r"launch_part<([^>]*)>\(MRS_LAUNCH_PASS\)")
    single = _parts((HIP / "step.hip").read_text(), r"(?m)^MRS_PART\(([^)]*)\);")
    assert sorted(set(launched)) == sorted(built), "launch_step names a part that build.py does not build, or misses one"
    assert single == built, "step.hip's single-unit instantiations are not build.py STEP_PARTS in its order"
