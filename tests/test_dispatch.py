"""The dispatch rule -- which kernel runs for (model, kernel_variant, N, dtype, B) -- is one host function, kmpc_select (csrc/kmpc_dispatch.h), which
kmpc_create, solve_dev and debug_kkt of kmpc_api.hip all ask.  CPU only: a few-line driver that includes the header is compiled with the HOST
compiler (the header's first part is plain C++17) and prints the selection on a grid of configurations; the expected values are written out here and
in bench.kernel_name (the statement of the rule the roofline is priced with), never taken from the function under test."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "csrc")
CXX = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)

BATCHES = (1, 1023, 1024, 2048, 2049, 262144)
DRIVER = r"""
#include <stdio.h>
#include "kmpc_dispatch.h"
int main()
{
    static const char *name[] = {"none", "generic", "fast", "wide", "quad"};
    const int batches[] = {%s};
    for (int model = 0; model <= 1; ++model)
        for (int variant = 0; variant <= 3; ++variant)
            for (int N = 2; N <= 56; ++N)
                for (int f64 = 1; f64 >= 0; --f64)
                    for (int B : batches) {
                        const kmpc_selection s = kmpc_select(model, variant, N, f64 != 0, B);
                        printf("%%d %%d %%d %%s %%d %%s %%d %%d\n", model, variant, N, f64 ? "f64" : "f32", B, name[s.backend], (int)s.dense,
                               (int)kmpc_selectable(model, variant, N, f64 != 0));
                    }
    return 0;
}
""" % ", ".join(str(b) for b in BATCHES)

F = (8, 12, 16, 20, 24, 28)            # one wave per problem
W = (32, 36, 40, 44, 48, 50)           # four waves per problem
# (back-end, model, dense) -> kernel; the generic and the four-per-wave kernels carry no horizon in their name
STEM = {("generic", 0, 0): "kmpc_solve_kernel", ("generic", 1, 0): "kmpc_solve_frenet_kernel",
        ("fast", 0, 0): "kmpc_solve_fast_kernel", ("fast", 0, 1): "kmpc_solve_fast_dense_kernel", ("fast", 1, 0): "kmpc_solve_fast_frenet_kernel",
        ("wide", 0, 0): "kmpc_solve_wide_kernel", ("wide", 1, 0): "kmpc_solve_wide_frenet_kernel",
        ("quad", 0, 0): "kmpc_solve_quad_kernel", ("quad", 1, 0): "kmpc_solve_quad_frenet_kernel"}


def kernel_of(backend, model, dense, N, dtype):
    if backend == "none":
        return None
    t = "double" if dtype == "f64" else "float"
    stem = STEM[(backend, model, dense)]   # KeyError: a combination no kernel exists for (a dense Frenet build, ...)
    return "%s<%s>" % (stem, t) if backend in ("generic", "quad") else "%s<%s,%d>" % (stem, t, N)


def expected(model, variant, N, dtype, B):
    """the table of the rule, row by row; None = refused by kmpc_create"""
    t = "double" if dtype == "f64" else "float"
    if model == 0:
        if variant == 3:
            return None
        if variant == 1:
            return "kmpc_solve_kernel<%s>" % t
        if variant == 0 and N == 8 and B >= 1024:
            return "kmpc_solve_quad_kernel<%s>" % t
        if N in F:
            return ("kmpc_solve_fast_dense_kernel<%s,%d>" if N <= 12 and B > 2048 else "kmpc_solve_fast_kernel<%s,%d>") % (t, N)
        if N in W:
            return "kmpc_solve_wide_kernel<%s,%d>" % (t, N)
        return "kmpc_solve_kernel<%s>" % t
    if variant == 3:
        return "kmpc_solve_quad_frenet_kernel<%s>" % t if N == 8 else None
    if variant == 1:
        return "kmpc_solve_frenet_kernel<%s>" % t if N <= 24 else None
    if N in F:
        return "kmpc_solve_fast_frenet_kernel<%s,%d>" % (t, N)
    if N in W:
        return "kmpc_solve_wide_frenet_kernel<%s,%d>" % (t, N) if dtype == "f64" else None
    return "kmpc_solve_frenet_kernel<%s>" % t if N <= 24 else None


@pytest.fixture(scope="module")
def selection(tmp_path_factory):
    d = tmp_path_factory.mktemp("dispatch")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
    rows = {}
    for l in subprocess.check_output([exe], text=True).splitlines():
        model, variant, N, dtype, B, backend, dense, ok = l.split()
        rows[(int(model), int(variant), int(N), dtype, int(B))] = (kernel_of(backend, int(model), int(dense), int(N), dtype), bool(int(ok)))
    assert len(rows) == 2 * 4 * 55 * 2 * len(BATCHES)
    return rows


pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


def test_default_variant_agrees_with_the_benchmarks_kernel_name(selection):
    sys.path.insert(0, ROOT)
    import bench
    pts = [k for k in selection if k[0] == 0 and k[1] == 0]
    assert len(pts) == 660
    bad = [(k, selection[k][0], bench.kernel_name(k[2], k[3], k[4])) for k in pts if selection[k][0] != bench.kernel_name(k[2], k[3], k[4])]
    assert not bad, bad[:5]


def test_selection_is_the_table(selection):
    bad = [(k, got, expected(*k)) for k, (got, _) in selection.items() if got != expected(*k)]
    assert not bad, bad[:5]


def test_create_accepts_exactly_what_has_a_kernel(selection):
    """kmpc_create asks kmpc_selectable; it must say yes exactly when every batch size finds a kernel -- in the table and in the function"""
    src = open(os.path.join(CSRC, "kmpc_api.hip")).read()
    create = src[src.index('extern "C" int32_t kmpc_create('):src.index('extern "C" int32_t kmpc_destroy(')]
    assert re.search(r"if \(!kmpc_selectable\(cfg->model, cfg->kernel_variant, cfg->N, cfg->dtype == KMPC_F64\)\)", create)
    assert "_available" not in src   # no second statement of the rule next to it
    for (model, variant, N, dtype, B), (got, ok) in selection.items():
        by_table = all(expected(model, variant, N, dtype, b) is not None for b in BATCHES)
        by_function = all(selection[(model, variant, N, dtype, b)][0] is not None for b in BATCHES)
        assert ok == by_table == by_function, (model, variant, N, dtype)
    # the parent's conditions, restated: 880 configurations
    for model in (0, 1):
        for variant in range(4):
            for N in range(2, 57):
                for dtype in ("f64", "f32"):
                    refused = (model == 1 and N > 24 and not (variant != 1 and (N == 28 or N in W))) or (variant == 3 and (model != 1 or N != 8)) or \
                              (model == 1 and N > 28 and dtype != "f64")
                    assert selection[(model, variant, N, dtype, 1)][1] == (not refused), (model, variant, N, dtype)
