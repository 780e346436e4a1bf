"""Records tests/golden/factor_step_parent.npz (tests/test_factor_step.py): outputs of 64 problems of bench draw 0, bit patterns of the build that is
loaded -- run it from the commit whose outputs a later change has to reproduce, before that change.

  python tools/record_factor_step_golden.py record [OUT.npz]    u0, cost, iters, status of the 64 rows: N = 20 in fp64 and fp32, N = 8 and N = 28 in fp64
  python tools/record_factor_step_golden.py retries             needs `make -C mkz_mpc_path_follower_amd/csrc trace`: factorisation retries of the five
                                                                named rows at N = 20 fp64 (per iteration: the attempt index of the factorisation that succeeded)

Rows: the slowest problem of the draw (1693) and four more long ones (533, 273, 1330, 3694), then 59 evenly spaced rows.  The inputs are rows of
make_batch(4096, N, cfg_id=2, seed=20180620 + 2), regenerated per horizon; they are solved as one batch of 64 (results do not depend on the batch)."""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 20180620 + 2
NAMED = (1693, 533, 273, 1330, 3694)
ROWS = np.array(NAMED + tuple(7 + 69 * k for k in range(59)), dtype=np.int64)
CASES = (("N20_f64", 20, False), ("N20_f32", 20, True), ("N8_f64", 8, False), ("N28_f64", 28, False))
KEYS = ("u0", "cost", "iters", "status")
assert len(set(ROWS.tolist())) == 64


def inputs(N, f32):
    from mkz_mpc_path_follower_amd.synthetic import make_batch
    d = make_batch(4096, N, cfg_id=2, seed=SEED, dtype=np.float32 if f32 else np.float64)
    return {k: np.ascontiguousarray(d[k][ROWS]) for k in ("z0", "ref", "v_target", "u_prev")}


def solve_case(N, f32):
    import torch
    from mkz_mpc_path_follower_amd import _lib
    if os.environ.get("KMPC_LIB"):   # (as the other tools: another build of the library)
        _lib.LIB_PATH = os.path.abspath(os.environ["KMPC_LIB"])
    from mkz_mpc_path_follower_amd import BatchMPC
    d = inputs(N, f32)
    s = BatchMPC(N=N, dtype=torch.float32 if f32 else torch.float64)
    o = s.solve(d["z0"], d["ref"], d["v_target"], d["u_prev"])
    torch.cuda.synchronize()
    r = {k: o[k].cpu().numpy() for k in KEYS}
    s.close()
    return r


def record(path):
    out = {"rows": ROWS}
    for name, N, f32 in CASES:
        r = solve_case(N, f32)
        for k in KEYS:
            out[name + "_" + k] = r[k]
        print("%-8s iters mean %.2f max %d (row %d), not Optimal %d" % (name, r["iters"].mean(), r["iters"].max(), ROWS[int(r["iters"].argmax())],
                                                                         int((r["status"] != 0).sum())), flush=True)
    if os.path.exists(path):  # keep the retry counts of an earlier `retries` run
        old = np.load(path)
        for k in old.files:
            if k.startswith("retries"):
                out[k] = old[k]
    np.savez(path, **out)
    print("wrote", path)


def retries(path):
    import ctypes as C
    import torch
    from mkz_mpc_path_follower_amd import _lib
    _lib.LIB_PATH = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "libkmpc_hip_trace.so")
    from mkz_mpc_path_follower_amd import BatchMPC
    d = inputs(20, False)
    s = BatchMPC(N=20)
    L = _lib.load()
    tr = torch.zeros((256, 8), dtype=torch.float64, device="cuda")
    L.kmpc_debug_set_stamps.argtypes = [C.c_void_p]
    L.kmpc_debug_set_stamps(C.c_void_p(tr.data_ptr()))
    counts = []
    for j in range(len(NAMED)):
        tr.zero_()
        o = s.solve(d["z0"][j:j + 1], d["ref"][j:j + 1], d["v_target"][j:j + 1], d["u_prev"][j:j + 1])
        torch.cuda.synchronize()
        it = int(o["iters"][0])
        att = tr.cpu().numpy()[129:129 + min(it, 127), 4].astype(np.int64)
        counts.append(int(att.sum()))
        print("row %4d: %2d iterations, %2d factorisation retries, per iteration %s" % (NAMED[j], it, counts[-1], att.tolist()), flush=True)
    L.kmpc_debug_set_stamps(None)
    if os.path.exists(path):
        old = dict(np.load(path))
        old["retries_named_N20_f64"] = np.array(counts, dtype=np.int64)
        np.savez(path, **old)
        print("added retries_named_N20_f64 to", path)


if __name__ == "__main__":
    default = os.path.join(ROOT, "tests", "golden", "factor_step_parent.npz")
    if len(sys.argv) >= 2 and sys.argv[1] == "record":
        record(sys.argv[2] if len(sys.argv) > 2 else default)
    elif len(sys.argv) >= 2 and sys.argv[1] == "retries":
        retries(sys.argv[2] if len(sys.argv) > 2 else default)
    else:
        sys.exit(__doc__)
