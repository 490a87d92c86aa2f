"""CPU: the plan of a guided trajectory (csrc/guidance_plan.h).  tests/host/guidance_plan.hip - a stand-alone program (its own main) that includes
the header and links nothing of the engine - is built here for the host, under address + undefined sanitizers where the toolchain links them,
and run: for every form, what each evaluation issues against the decision rules of the code before the plan existed, the floats that travel
behind the stage times against the former count and copies, and that filling them writes exactly that many."""
import os
import subprocess

import pytest

from test_threads_cpu import CSRC, REPO, REPORT_MARKS, _hipcc

HOST_SRC = os.path.join(REPO, "tests", "host", "guidance_plan.hip")


def test_guidance_plan_host_program(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    log = []
    for san in ("address,undefined", None):  # (a runtime the toolchain lacks fails at the link)
        exe = os.path.join(str(tmp_path), "guidance_plan_" + ("san" if san else "plain"))
        cmd = [hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, HOST_SRC, "-o", exe]
        if san:
            cmd += ["-Xarch_host", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
        log.append(f"$ {' '.join(cmd)}\n{r.stdout}{r.stderr}")
        if r.returncode == 0 and os.path.exists(exe):
            break
    else:
        raise AssertionError("tests/host/guidance_plan.hip does not build, with or without a sanitizer:\n" + "\n".join(log))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    print(f"guidance_plan built with sanitizer: {san or 'none (no sanitizer runtime links here)'}\n{out}")
    assert r.returncode == 0, out
    assert "guidance_plan: ok" in r.stdout
    for mark in REPORT_MARKS:
        assert mark not in out, f"sanitizer report ({mark}):\n{out}"
