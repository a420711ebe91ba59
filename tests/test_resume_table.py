"""The workgroup table of the fleet's resume launch (csrc/resume_table.h: counts, cpw, W -> table, grid) on the CPU, before any device
run: a mistake there is an out-of-range read on the device. The header has no HIP in it; tests/resume_table_check.cc wraps it in a shared
object (as tests/quademu does for the step function). Every table is walked as rollout_quad_resume_kernel walks it: workgroup b serves
slots first + w * cpw + quad (w < W, quad < cpw) of environment env's list while they are below its count."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPWS, WS = (1, 2, 4, 8, 16), (1, 4)


@pytest.fixture(scope="module")
def rt(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resume_table") / "libresume_table.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", so, os.path.join(HERE, "resume_table_check.cc")])
    L = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    L.rt_cpw.argtypes, L.rt_cpw.restype = [C.c_longlong], C.c_int
    L.rt_waves.argtypes, L.rt_waves.restype = [ip, C.c_int, C.c_int], C.c_longlong
    L.rt_wpg.argtypes, L.rt_wpg.restype = [C.c_longlong], C.c_int
    L.rt_build.argtypes, L.rt_build.restype = [ip, C.c_int, C.c_int, C.c_int, ip, C.c_longlong], C.c_longlong
    return L


def build(rt, counts, cpw, W, cap=None):
    counts = np.ascontiguousarray(counts, np.int32)
    ip = C.POINTER(C.c_int)
    grid = rt.rt_build(counts.ctypes.data_as(ip), len(counts), cpw, W, None, 0)
    if grid < 0:
        return grid, None
    cap = grid if cap is None else cap
    guard = 8   # ints behind the table that must stay untouched
    table = np.full(4 * max(cap, 0) + guard, -77, np.int32)
    got = rt.rt_build(counts.ctypes.data_as(ip), len(counts), cpw, W, table.ctypes.data_as(ip), cap)
    assert (table[4 * max(cap, 0):] == -77).all()
    return got, table[:4 * max(cap, 0)].reshape(-1, 4)


def walk(counts, cpw, W, grid, table):
    """-> per environment, how often each slot of its list is served"""
    served = [np.zeros(c, int) for c in counts]
    assert len(table) == grid
    for env, first, count, _ in table:
        assert 0 <= env < len(counts) and count == counts[env]
        assert 0 <= first < count          # no workgroup is wholly empty, none starts past its environment's count
        assert first % (cpw * W) == 0
        for w in range(W):
            for quad in range(cpw):
                slot = first + w * cpw + quad
                if slot < count:           # (the kernel's own check; a slot past the count is never read)
                    served[env][slot] += 1
    return served


CASES = [[0], [1], [64], [0, 5, 7], [5, 7, 0], [0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0], [63, 1, 17], [64, 64, 64], [3, 66, 130], [2048, 0, 2047, 1],
         [65, 129, 3, 0, 31], [57, 60, 48], [7, 4, 16]]


@pytest.mark.parametrize("cpw,W", list(itertools.product(CPWS, WS)))
def test_every_listed_candidate_is_served_exactly_once_by_a_workgroup_of_its_environment(rt, cpw, W):
    rng = np.random.default_rng(100 * cpw + W)
    cases = CASES + [list(np.where(rng.random(E) < 0.3, 0, rng.integers(1, 400, E))) for E in rng.integers(1, 12, 40)]
    for counts in cases:
        grid, table = build(rt, counts, cpw, W)
        # the grid is the sum of the environments' own workgroup counts: never a workgroup across two environments
        assert grid == sum(-(-(-(-c // cpw)) // W) for c in counts), counts
        for e, s in enumerate(walk(counts, cpw, W, grid, table)):
            assert (s == 1).all(), (counts, e)
        # the entries are environment-major, an environment's in slot order
        assert [tuple(r[:2]) for r in table] == sorted(tuple(r[:2]) for r in table)


@pytest.mark.parametrize("cpw,W", list(itertools.product(CPWS, WS)))
def test_one_environment_is_the_plain_resume_launch(rt, cpw, W):
    for n in (1, 2, 3, cpw, cpw + 1, cpw * W, cpw * W + 1, 127, 1024, 4097):
        grid, table = build(rt, [n], cpw, W)
        waves = (n + cpw - 1) // cpw
        assert grid == (waves + W - 1) // W       # launch_resume_quad's grid
        assert (table[:, 0] == 0).all() and np.array_equal(table[:, 1], np.arange(grid) * cpw * W) and (table[:, 2] == n).all()


def test_the_launch_shape_helpers_match_the_plain_path(rt):
    def plain_cpw(n):   # launch_resume_quad as it was before the table: from 16 down to one while the halved width still fits 1024 wavefronts
        cpw = 16
        while cpw > 1 and (n + cpw // 2 - 1) // (cpw // 2) <= 1024:
            cpw >>= 1
        return cpw
    for n in (1, 2, 63, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384):
        assert rt.rt_cpw(n) == plain_cpw(n), n
    assert [rt.rt_wpg(w) for w in (1, 1023, 1024, 5000)] == [1, 1, 4, 4]
    counts = np.array([5, 0, 9, 16], np.int32)
    assert rt.rt_waves(counts.ctypes.data_as(C.POINTER(C.c_int)), 4, 4) == 2 + 0 + 3 + 4


def test_a_table_that_does_not_fit_and_bad_arguments_are_refused(rt):
    counts = [5, 7, 3]
    grid, _ = build(rt, counts, 2, 1)
    assert grid == 3 + 4 + 2
    for cap in (0, 1, grid - 1):
        got, _ = build(rt, counts, 2, 1, cap=cap)
        assert got == -1
    assert build(rt, [3, -1], 4, 1)[0] == -1
    assert build(rt, [3], 0, 1)[0] == -1 and build(rt, [3], 4, 0)[0] == -1
    assert build(rt, [0, 0], 4, 4)[0] == 0
