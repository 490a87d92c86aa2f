"""CPU: what the library promises about threads, as far as it can be checked without a device.

1. tests/host/options_threads.hip - a stand-alone program (its own main) that links csrc/options.hip and nothing else of the engine - is
   built here with a host sanitizer where the toolchain ships one (thread, else address + undefined, else none) and run: snapshot
   constancy of LtOptScope, its generations-first ordering rule, thread locality and nesting, override resolution under change.
2. lt_last_error() is thread-local: two Python threads provoke two different refusals (ctypes releases the GIL in the calls) and each
   reads its own message back, every time.
3. the prompt cache of a DiTEngine survives clear() from another thread (what set_option does) while hit() runs.
"""
import ctypes as C
import os
import shutil
import subprocess
import threading

import pytest
import torch

import lumina_t2x_amd  # noqa: F401  (import shim)
from lumina_t2x_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lumina-t2x_amd", "csrc")
HOST_SRC = os.path.join(REPO, "tests", "host", "options_threads.hip")
SANITIZERS = ("thread", "address,undefined", None)
REPORT_MARKS = ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "UndefinedBehaviorSanitizer", "runtime error:")
JOIN_TIMEOUT = 300.0


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _build_host_program(hipcc, out_dir):
    """the program under the first sanitizer that compiles and links (a runtime the toolchain lacks fails at the link); returns
    (path, sanitizer or None)"""
    log = []
    for san in SANITIZERS:
        exe = os.path.join(out_dir, "options_threads_" + (san or "plain").replace(",", "_"))
        # host code only: the two sources hold no kernel
        cmd = [hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-pthread", "-I", CSRC, HOST_SRC, os.path.join(CSRC, "options.hip"), "-o", exe]
        if san:
            cmd += ["-Xarch_host", f"-fsanitize={san}", "-fno-omit-frame-pointer"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=out_dir)
        log.append(f"$ {' '.join(cmd)}\n{r.stdout}{r.stderr}")
        if r.returncode == 0 and os.path.exists(exe):
            return exe, san
    raise AssertionError("tests/host/options_threads.hip does not build, with or without a sanitizer:\n" + "\n".join(log))


def test_option_scope_under_threads_host_program(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    exe, san = _build_host_program(hipcc, str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    print(f"options_threads built with sanitizer: {san or 'none (no sanitizer runtime links here)'}\n{out}")
    assert r.returncode == 0, out
    assert "options_threads: ok" in r.stdout
    for mark in REPORT_MARKS:
        assert mark not in out, f"sanitizer report ({mark}):\n{out}"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _run_threads(workers):
    """start together, collect what the workers raise, fail on a join that expires"""
    barrier = threading.Barrier(len(workers))
    errors = []

    def wrap(fn):
        def go():
            try:
                barrier.wait(JOIN_TIMEOUT)
                fn()
            except BaseException as exc:  # noqa: BLE001 - re-raised on the main thread
                errors.append(exc)
        return go

    threads = [threading.Thread(target=wrap(fn), daemon=True) for fn in workers]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_TIMEOUT)
        assert not t.is_alive(), "a worker did not finish"
    if errors:
        raise errors[0]


def test_last_error_is_thread_local(lib):
    n = 4000
    seen = {"range": set(), "unknown": set()}

    def out_of_range():
        for _ in range(n):
            assert lib.lt_set_option(b"gemm_splitk", 7) != 0
            seen["range"].add(lib.lt_last_error())

    def unknown_name():
        v = C.c_int32(0)
        for _ in range(n):
            assert lib.lt_engine_get_option(None, b"no_such", C.byref(v)) != 0
            seen["unknown"].add(lib.lt_last_error())

    _run_threads([out_of_range, unknown_name])
    assert seen["range"] == {b"option gemm_splitk must be 0 .. 2 (got 7)"}, seen["range"]
    assert seen["unknown"] == {b"lt_engine_get_option: unknown option 'no_such'"}, seen["unknown"]
    # a thread that never failed reads the empty message, not a neighbour's
    fresh = []
    t = threading.Thread(target=lambda: fresh.append(lib.lt_last_error()))
    t.start()
    t.join(JOIN_TIMEOUT)
    assert fresh == [b""], fresh
    v = C.c_int32(-1)  # and nothing stuck: the refused value never became the default
    assert lib.lt_engine_get_option(None, b"gemm_splitk", C.byref(v)) == 0 and v.value == 1


def test_prompt_cache_hit_survives_clear_from_another_thread():
    """DiTEngine.set_option clears the engine's prompt cache; a sampler thread is inside hit() / store() meanwhile.  Any interleaving is a
    hit or a miss, never an exception (the round-trip itself - which tensors count as a hit - is tests/test_host_logic.py's)"""
    from lumina_t2x_amd.engine import _SourceCache
    cache = _SourceCache()
    a, b = torch.zeros(2, 3), torch.ones(2, dtype=torch.int32)
    n = 20000
    hits = [0]
    done = threading.Event()

    def sampler():
        try:
            for _ in range(n):
                if cache.hit((a, b), ("prompt",)):
                    hits[0] += 1
                else:
                    cache.store((a, b), ("prompt",))
        finally:
            done.set()

    def setter():
        while not done.is_set():
            cache.clear()

    _run_threads([sampler, setter])
    cache.store((a, b), ("prompt",))
    assert cache.hit((a, b), ("prompt",)) and not cache.hit((a, b), ("labels",)) and not cache.hit((b, a), ("prompt",))
    print(f"prompt cache: {hits[0]} hits of {n} under clear() from a second thread")
