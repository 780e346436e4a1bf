"""Static budget of the headline kernels (CPU only: hipcc cross-compiles kmpc_fast.hip for gfx950 as tests/test_codegen.py does, nothing runs).

The B = 4096 headline lasts as long as its slowest problem, whose wave spends most of its life alone on its SIMD: there every instruction
and every LDS round trip it waits out adds to the launch.  The ceilings sit a few per cent above what the shipped
source compiles to (tools/static_mix.py prints the same counts), so that overhead cannot creep back unnoticed; occupancy, scratch and LDS
must stay what the launch bounds were chosen for."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRC = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "csrc", "kmpc_fast.hip")

# kernel: (static VALU, SGPR spills, exec-mask regions, s_waitcnt, waves per CU)
BUDGET = {"kmpc_solve_fast_kernel<double, 20>": (5700, 82, 278, 345, 8),
          "kmpc_solve_fast_kernel<float, 20>": (4250, 50, 295, 285, 16)}


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    import static_mix as M
    return {r["kernel"]: r for r in M.analyse(SRC, list(BUDGET))}


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_headline_kernel_within_budget(rows, kernel):
    valu, sspill, execr, waits, wpc = BUDGET[kernel]
    r = rows[kernel]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["valu"] <= valu, r
    assert r["sgpr_spill"] <= sspill, r
    assert r["exec_regions"] <= execr, r
    assert r["waitcnt"] <= waits, r
    assert r["waves_per_cu"] == wpc, r
    assert r["lds"] <= 20480, r
