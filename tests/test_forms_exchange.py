"""The constraint forms of the one-wave fp64 kernels with three tile rows (N = 16, 20): forms_apply / forms_applyT request every LDS word a lane needs
behind one wait, with clamped addresses and selects instead of exec-masked arms (kmpc_ipm.h, FORMS_AHEAD).  What that can break is a stale wb / cb / xb
word read ahead of its store, and the lanes >= n and forms >= nf whose addresses are clamped -- either shows as different iterates, so the one-wave kernel
is held against

  * the generic kernel (kernel_variant = 1, its own forms code): same statuses, costs to 1e-7 relative and mean iteration counts within 0.5 -- what
    tests/test_gpu_parity.py::test_fast_and_generic_kernels_agree asks of the two; first input to 1e-6, violation <= 1e-8 + 1e-12 and X to 1e-4 -- what
    that file asks of one solve against another of the same algorithm with a different summation order; U to 1e-4 like the predictions it produces;
  * the per-problem-parameter entry point with the handle's own weights and limits (kmpc_solve_batch_params: the `_par` twin of the same kernel, which
    must compile the same forms): every output bit for bit;

cold, warm-started from the previous plan, and at B = 1.  All solves of a horizon are made once and shared."""
import numpy as np
import pytest
import torch

from mkz_mpc_path_follower_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu

KEYS = ("u0", "U", "X", "status", "iters", "cost", "viol")
B = 256


def _np(o):
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy().copy() for k in KEYS}


@pytest.fixture(scope="module", params=[16, 20])
def runs(request):
    from mkz_mpc_path_follower_amd import BatchMPC
    N = request.param
    d = make_batch(B, N, cfg_id=2, seed=7100 + N)
    one = {k: d[k][:1] for k in ("z0", "ref", "v_target", "u_prev")}
    out = {"N": N}
    for name, kv, par in (("plain", 0, False), ("generic", 1, False), ("params", 0, True)):
        s = BatchMPC(N=N, kernel_variant=kv)
        args = (d["z0"], d["ref"], d["v_target"], d["u_prev"])
        p = s.problem_params(B) if par else None
        cold = _np(s.solve(*args, want_U=True, want_X=True, params=p))
        W = torch.as_tensor(cold["U"], device="cuda").clone()   # (the kernel writes the new plan back into the warm-start buffer)
        warm = _np(s.solve(*args, warm_U=W, warm=True, want_U=True, want_X=True, params=p))
        single = _np(s.solve(one["z0"], one["ref"], one["v_target"], one["u_prev"], want_U=True, want_X=True, params=p[:1] if par else None))
        out[name] = {"cold": cold, "warm": warm, "single": single}
        s.close()
    return out


def _close(a, b, tag):
    rel = np.abs(a["cost"] - b["cost"]) / np.maximum(1.0, np.abs(b["cost"]))
    fig = dict(cost_rel=rel.max(), u0=np.abs(a["u0"] - b["u0"]).max(), U=np.abs(a["U"] - b["U"]).max(), X=np.abs(a["X"] - b["X"]).max(),
               viol=max(a["viol"].max(), b["viol"].max()), iters=(a["iters"].mean(), b["iters"].mean()), bad=int((a["status"] != 0).sum() + (b["status"] != 0).sum()))
    print(tag, fig)
    assert (a["status"] == 0).all() and (b["status"] == 0).all(), fig
    assert rel.max() <= 1e-7, fig
    assert abs(a["iters"].mean() - b["iters"].mean()) < 0.5, fig
    assert fig["u0"] <= 1e-6 and fig["U"] <= 1e-4 and fig["X"] <= 1e-4, fig
    assert fig["viol"] <= 1e-8 + 1e-12, fig


def _same(a, b, tag):
    diff = [k for k in KEYS if not np.array_equal(a[k], b[k])]
    print(tag, "differing outputs:", diff)
    assert not diff, diff


def test_one_wave_kernel_agrees_with_the_generic_kernel(runs):
    _close(runs["plain"]["cold"], runs["generic"]["cold"], "N=%d cold" % runs["N"])


def test_params_twin_is_bit_identical(runs):
    _same(runs["plain"]["cold"], runs["params"]["cold"], "N=%d cold" % runs["N"])


def test_warm_started_call(runs):
    _close(runs["plain"]["warm"], runs["generic"]["warm"], "N=%d warm" % runs["N"])
    _same(runs["plain"]["warm"], runs["params"]["warm"], "N=%d warm" % runs["N"])
    assert runs["plain"]["warm"]["iters"].mean() < runs["plain"]["cold"]["iters"].mean()


def test_single_problem_call(runs):
    _close(runs["plain"]["single"], runs["generic"]["single"], "N=%d B=1" % runs["N"])
    _same(runs["plain"]["single"], runs["params"]["single"], "N=%d B=1" % runs["N"])
    _same(runs["plain"]["single"], {k: v[:1] for k, v in runs["plain"]["cold"].items()}, "N=%d B=1 against row 0 of the batch" % runs["N"])
