"""CPU: the kinds of a model evaluation (csrc/eval_kind.h).  tests/host/eval_kind.hip - a stand-alone program (its own main) that includes the
header and links nothing of the engine - is built here for the host, under address + undefined sanitizers where the toolchain links them, and
run: every kind's traits against the rules of the code before the kinds had names, and the kernel modes of the three skip-layer kinds."""
import os
import subprocess

import pytest

from test_threads_cpu import CSRC, REPO, REPORT_MARKS, _hipcc

HOST_SRC = os.path.join(REPO, "tests", "host", "eval_kind.hip")


def test_eval_kind_traits_host_program(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    log = []
    for san in ("address,undefined", None):  # (a runtime the toolchain lacks fails at the link)
        exe = os.path.join(str(tmp_path), "eval_kind_" + ("san" if san else "plain"))
        cmd = [hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, HOST_SRC, "-o", exe]
        if san:
            cmd += ["-Xarch_host", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
        log.append(f"$ {' '.join(cmd)}\n{r.stdout}{r.stderr}")
        if r.returncode == 0 and os.path.exists(exe):
            break
    else:
        raise AssertionError("tests/host/eval_kind.hip does not build, with or without a sanitizer:\n" + "\n".join(log))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    print(f"eval_kind built with sanitizer: {san or 'none (no sanitizer runtime links here)'}\n{out}")
    assert r.returncode == 0, out
    assert "eval_kind: ok" in r.stdout
    for mark in REPORT_MARKS:
        assert mark not in out, f"sanitizer report ({mark}):\n{out}"
