"""Bit-identity check of two library builds: every output array of seeded draws over the solve kernels, compared with np.array_equal.

  KMPC_LIB=a.so python tools/output_digest.py save DIR_A      solve the draws with build a, write DIR_A/<draw>.npz
  python tools/output_digest.py compare DIR_A DIR_B          exit code 1 if any element of any array differs

Draws: bench.py's four draws (B = 4096, N = 20, fp64, cfg_id 2, seeds 20180622 + 7919 j); B = 262 144 at N = 20 in fp64 and fp32;
N = 8 .. 28 in both precisions at B = 512 (the one-wave kernel: at N = 8 batches of 1024 or more go to the quad kernel); the three-waves-per-SIMD
build of N = 8 and 12 (B = 4096, kernel_variant 2 keeps N = 8 off the quad kernel); N = 50 (four-wave kernel); the quad kernel (N = 8,
B = 4096); the Frenet functor at N = 16 and 20; the generic kernel in both models (N = 10, B = 512); the four-wave Frenet kernel (N = 32, B = 512); the
four-per-wave Frenet kernel with a partial last wave (N = 8, kernel_variant 3, B = 4099); N = 20 through per-problem parameters (eight interleaved sets of
synthetic.make_param_sets); N = 20 in fp32 through packed records at B = 4096 (pack / solve_packed, behind the start-order pre-pass)."""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("u0", "U", "X", "status", "iters", "cost", "viol")


def draws():
    d = [("bench_d%d" % j, dict(N=20, B=4096, f32=False, seed=20180620 + 2 + 7919 * j)) for j in range(4)]
    d += [("big_f64", dict(N=20, B=262144, f32=False, seed=4)), ("big_f32", dict(N=20, B=262144, f32=True, seed=4))]
    for N in (8, 12, 16, 24, 28):
        for f32 in (False, True):
            d.append(("N%d_%s" % (N, "f32" if f32 else "f64"), dict(N=N, B=512, f32=f32, seed=5)))
    for N in (8, 12):
        for f32 in (False, True):
            d.append(("N%d_%s_dense" % (N, "f32" if f32 else "f64"), dict(N=N, B=4096, f32=f32, seed=9, opts=dict(kernel_variant=2))))
    d.append(("N50_wide", dict(N=50, B=4096, f32=False, seed=6, cfg=5)))
    d.append(("N8_quad", dict(N=8, B=4096, f32=False, seed=7)))
    for N in (16, 20):
        d.append(("frenet_N%d" % N, dict(N=N, B=4096, f32=False, seed=8, frenet=True)))
    d.append(("N10_generic", dict(N=10, B=512, f32=False, seed=10)))
    d.append(("frenet_N10_generic", dict(N=10, B=512, f32=False, seed=11, frenet=True)))
    d.append(("frenet_N32_wide", dict(N=32, B=512, f32=False, seed=12, frenet=True)))
    d.append(("frenet_N8_quad", dict(N=8, B=4099, f32=False, seed=13, frenet=True, opts=dict(kernel_variant=3))))
    d.append(("N20_params", dict(N=20, B=4096, f32=False, seed=14, param_sets=8)))
    d.append(("N20_f32_packed", dict(N=20, B=4096, f32=True, seed=15, packed=True)))
    return d


def frenet_cases(B, seed):
    rng = np.random.default_rng(seed)
    z0 = np.stack([rng.uniform(0, 5, B), rng.normal(0, 0.4, B), rng.normal(0, 0.08, B), rng.uniform(2, 12, B)], 1)
    a, b, c, d = rng.uniform(-0.04, 0.04, B), rng.normal(0, 0.015, B), rng.normal(0, 0.015, B), rng.normal(0, 0.015, B)
    kp = np.stack([d / 60.0 ** 3, c / 60.0 ** 2, b / 60.0, a], 1)
    vt = np.clip(z0[:, 3] + rng.normal(0, 1.0, B), 1.0, 15.0)
    up = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.05, 0.05, B)], 1)
    return z0, kp, vt, up


def save(outdir):
    import torch
    from mkz_mpc_path_follower_amd import _lib
    if os.environ.get("KMPC_LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["KMPC_LIB"])
    from mkz_mpc_path_follower_amd import BatchMPC
    from mkz_mpc_path_follower_amd.synthetic import apply_param_sets, make_batch, make_param_sets
    os.makedirs(outdir, exist_ok=True)
    for name, p in draws():
        dt = torch.float32 if p["f32"] else torch.float64
        npdt = np.float32 if p["f32"] else np.float64
        if p.get("frenet"):
            z0, kp, vt, up = (np.ascontiguousarray(x, dtype=npdt) for x in frenet_cases(p["B"], p["seed"]))
            s = BatchMPC(N=p["N"], dtype=dt, model=1, **p.get("opts", {}))
            o = s.solve_frenet(z0, kp, vt, up, want_U=True, want_X=True)
        else:
            d = make_batch(p["B"], p["N"], cfg_id=p.get("cfg", 2), seed=p["seed"], dtype=npdt)
            rec = apply_param_sets(d, make_param_sets(p["param_sets"], p["seed"] + 1)) if p.get("param_sets") else None
            s = BatchMPC(N=p["N"], dtype=dt, **p.get("opts", {}))
            if p.get("packed"):
                o = s.solve_packed(s.pack(d["z0"], d["ref"], d["v_target"], d["u_prev"]), want_U=True, want_X=True)
            else:
                o = s.solve(d["z0"], d["ref"], d["v_target"], d["u_prev"], want_U=True, want_X=True, params=rec)
        torch.cuda.synchronize()
        r = {k: o[k].cpu().numpy() for k in KEYS if k in o}
        np.savez(os.path.join(outdir, name + ".npz"), **r)
        print("%-18s B=%-6d N=%-2d %s  iters mean %.3f max %d  not Optimal %d" % (name, p["B"], p["N"], "f32" if p["f32"] else "f64",
              r["iters"].mean(), r["iters"].max(), int((r["status"] != 0).sum())), flush=True)
        s.close()


def compare(da, db):
    bad = 0
    for name, _ in draws():
        a, b = np.load(os.path.join(da, name + ".npz")), np.load(os.path.join(db, name + ".npz"))
        diff = [k for k in a.files if not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]
        if sorted(a.files) != sorted(b.files):
            diff.append("keys")
        n = sum(int((a[k] != b[k]).sum()) for k in diff if k != "keys")
        print("%-18s %s" % (name, "identical (%s)" % " ".join(a.files) if not diff else "DIFFERS in %s (%d elements)" % (diff, n)))
        bad += bool(diff)
    print("draws that differ: %d" % bad)
    return bad


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "save":
        save(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    else:
        sys.exit(__doc__)
