"""CPU: the threaded host code — the plan build from 20 000 spins on (csrc/sa_plan.cpp: exact
symmetry confirmation, counting-sort transposition, two-pass merge, ELL fill, row quads), the
shuffled orders' and the greedy trees' thread pools.

Leg 1 builds the stand-alone checker tools/host_check/ plain, under the thread sanitizer and under
the address + undefined-behaviour sanitizers, and runs each binary directly.  Leg 2 goes through
the C ABI with ASP_HOST_THREADS unset, 1, 3 and 64 against the oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT
from host_thread_cases import FORMS, forms

VARIANTS = ("plain", "tsan", "asan")
SANITIZER_REPORT = re.compile(r"ThreadSanitizer|AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|"
                              r"MemorySanitizer|runtime error:")
NO_RUNTIME = re.compile(r"libclang_rt|cannot find -l(tsan|asan|ubsan)|lib(tsan|asan|ubsan)[^ ]*: No such file|"
                        r"unsupported option '-fsanitize|unsupported argument '[a-z,]+' to option '-fsanitize")


@pytest.fixture(scope="module")
def checker_runs(tmp_path_factory):
    """{variant: (exit code, output)} of `run.sh -o DIR variant` (build, then the binary run
    directly), the three side by side."""
    out = tmp_path_factory.mktemp("host_check")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASP_")}
    running = {}
    for variant in VARIANTS:
        log = open(out / (variant + ".log"), "w+")
        running[variant] = (subprocess.Popen(["bash", os.path.join(ROOT, "tools", "host_check", "run.sh"),
                                              "-o", str(out), variant], stdout=log, stderr=subprocess.STDOUT,
                                             stdin=subprocess.DEVNULL, env=env, cwd=ROOT), log)
    results = {}
    for variant, (process, log) in running.items():
        try:
            code = process.wait(timeout=900)
        except subprocess.TimeoutExpired:
            process.kill()
            process.wait()
            code = "timeout"
        log.seek(0)
        results[variant] = (code, log.read())
        log.close()
    return results


@pytest.mark.parametrize("variant", VARIANTS)
def test_host_checker(checker_runs, variant):
    code, output = checker_runs[variant]
    built = re.search(r"^built .*host_check_" + variant + "$", output, re.M)
    started = re.search(r"^host_check: ", output, re.M)
    tail = "\n".join(output.splitlines()[-25:])
    if variant != "plain":
        # a sanitizer build may be missing only where the instrumented binary cannot exist or
        # cannot start on this machine; the reason is the tool's own message
        if not built and NO_RUNTIME.search(output):
            pytest.skip("no %s runtime for this compiler: %s" % (variant, tail))
        if built and not started and code != 0:
            pytest.skip("the %s binary cannot start here: %s" % (variant, tail))
    assert built, "the %s build failed:\n%s" % (variant, tail)
    assert started, "no banner line from the %s build:\n%s" % (variant, tail)
    assert not SANITIZER_REPORT.search(output), "sanitizer report in the %s run:\n%s" % (variant, output[-6000:])
    assert code == 0, "the %s checker exited with %s:\n%s" % (variant, code, tail)
    checks = re.findall(r"^check (\S+) (.*)$", output, re.M)
    assert checks and all(state == "ok" for _, state in checks), tail
    # every check ran: thread counts against one thread, the reference, the structure, the
    # shuffled orders and the greedy batch, at both sides of the threshold and a ragged size
    names = {name for name, _ in checks}
    for n in (19999, 20000, 20011):
        for form in ("symmetric", "upper", "one_sided", "nudged", "holed"):
            for threads in (3, 4, 7, 64):
                assert "A.threads/%d/%s/%d" % (threads, form, n) in names
                assert "B.reference/%d-threads/%s/%d" % (threads, form, n) in names
            assert "C.structure/3-threads/%s/%d" % (form, n) in names
        assert "B.upper-equals-symmetric/upper/%d" % n in names
        assert "D.shuffled/one_sided/%d" % n in names and "D.shuffled/symmetric/%d" % n in names
    assert "E.greedy-many/40-layouts" in names
    assert output.rstrip().endswith("host_check: all checks ok")


def _host_run(lib, n, m, field):
    from annealing_sign_problem_amd import _lib

    indptr, indices = m.indptr.astype(np.int64), m.indices.astype(np.int32)
    args = (n, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(m.data), _lib.ptr(field))
    info = _lib.SaInfo()
    colors, pos = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    x = np.zeros((n + 63) // 64, np.uint64)
    _lib.check(lib.asp_sa_layout_host(*args, ctypes.byref(info), _lib.ptr(colors), _lib.ptr(pos)))
    _lib.check(lib.asp_sa_greedy_tree_host(*args, _lib.ptr(x)))
    orders = []
    for sweep in (0, 5):
        order, level = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        levels = ctypes.c_uint32(0)
        _lib.check(lib.asp_sa_shuffled_order_host(*args, 0x1234567890ABCDEF, sweep, _lib.ptr(order),
                                                  _lib.ptr(level), ctypes.byref(levels)))
        orders.append((order, level, levels.value))
    return info, colors, pos, x, orders


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [20000, 20011])
def test_plan_build_does_not_depend_on_the_host_threads(n, form, monkeypatch):
    """asp_sa_layout_host, asp_sa_greedy_tree_host and asp_sa_shuffled_order_host with
    ASP_HOST_THREADS unset (four threads), 1, 3 and 64: each run is what the oracle says, and the
    runs are equal to each other."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    matrices, field = forms(n)
    m = matrices[form]
    ocolors, oorder, ncol, nnz, diag = oracle.sa_layout(m)
    ox = oracle.greedy_solve(m, field, relax=False)[0]
    first = None
    for threads in (None, 1, 3, 64):
        if threads is None:
            monkeypatch.delenv("ASP_HOST_THREADS", raising=False)
        else:
            monkeypatch.setenv("ASP_HOST_THREADS", str(threads))
        info, colors, pos, x, orders = _host_run(lib, n, m, field)
        assert np.array_equal(colors, ocolors) and info.num_colors == ncol, threads
        assert np.all(np.diff(pos[oorder].astype(np.int64)) > 0), threads   # same visiting order
        assert info.nnz_offdiag == nnz and info.diag_sum == diag, threads
        assert np.array_equal(x, ox), threads
        if first is None:
            first = (info, pos, orders)
            continue
        assert np.array_equal(pos, first[1]), threads
        for name in ("beta0_auto", "beta1_auto", "energy_scale_exp"):
            assert getattr(info, name) == getattr(first[0], name), (threads, name)
        for (order, level, levels), (order1, level1, levels1) in zip(orders, first[2]):
            assert levels == levels1 and np.array_equal(order, order1) and np.array_equal(level, level1), threads
    assert sorted(first[2][0][0].tolist()) == list(range(n)) and first[2][0][2] > 1
    assert not np.array_equal(first[2][0][0], first[2][1][0])   # another sweep, another order


@pytest.mark.parametrize("n", [20000, 20011])
def test_upper_triangle_gives_the_symmetric_plan(n, monkeypatch):
    """The general merge of the upper triangle (threaded) gives the short cut's plan of the
    symmetric matrix, bit for bit."""
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    matrices, field = forms(n)
    monkeypatch.setenv("ASP_HOST_THREADS", "3")
    a = _host_run(lib, n, matrices["symmetric"], field)
    b = _host_run(lib, n, matrices["upper"], field)
    assert bytes(a[0]) == bytes(b[0])                      # every field of asp_sa_info
    for got, want in zip(a[1:4], b[1:4]):
        assert np.array_equal(got, want)
    for (order, level, levels), (order1, level1, levels1) in zip(a[4], b[4]):
        assert levels == levels1 and np.array_equal(order, order1) and np.array_equal(level, level1)
