"""Fuzz of cost weights x horizons x precisions on in-distribution and out-of-distribution states: every weight log-uniform over four decades around the node's
defaults (zero weights included with probability 0.3 each), B problems per setting; the GPU result against the CPU port problem by problem (cost within 1e-6 / 1e-3
relative, or both certified as different local minima).   usage: python tools/fuzz_weights.py [settings] [B] [--one-launch] [--horizon N] [--gpu-only] [--fp64-only]
(diagnostic; uses oracle/ as the checker).  Default: one fresh handle and one launch per setting and precision.  --one-launch: all settings of one horizon and
precision are packed into a single batch, each problem carrying its setting's weights in its `params` record (BatchMPC.solve(..., params=)).  --horizon N: every
setting at horizon N.  --gpu-only: skip the CPU port and the comparison (timing runs).  Both modes print the wall time of their GPU part."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import certify as CT
    from oracle import oracle as O
    from mkz_mpc_path_follower_amd import BatchMPC
    from mkz_mpc_path_follower_amd.synthetic import make_batch, make_ood_batch
    import time
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    one_launch, gpu_only = "--one-launch" in flags, "--gpu-only" in flags
    dtypes = (torch.float64,) if "--fp64-only" in flags else (torch.float64, torch.float32)
    fixed_N = None
    if "--horizon" in flags:   # (its value is the positional argument that follows it)
        fixed_N = int(sys.argv[sys.argv.index("--horizon") + 1])
        args.remove(str(fixed_N))
    S = int(args[0]) if len(args) > 0 else 24
    B = int(args[1]) if len(args) > 1 else 2048
    rng = np.random.default_rng(77)
    base = np.array([9.0, 9.0, 10.0, 1.0, 100.0, 1000.0, 1.0, 1.0])   # (C_v, C_acc, C_df default to 0: the fuzz draws them around 1)
    paths = [dict(np.load(os.path.join(ROOT, "tests", "golden", "path%d_decimated.npz" % k))) for k in (1, 2, 3)]
    tot = bad = 0
    gpu_s = 0.0
    settings = []
    for k in range(S):
        N = int(rng.choice([8, 12, 16, 20, 24, 28, 32, 40, 50]))
        w = base * 10.0 ** rng.uniform(-2, 2, 8)
        w[rng.uniform(size=8) < 0.3] = 0.0
        if w[:3].sum() == 0: w[0] = 9.0
        settings.append((k, fixed_N or N, w, k % 2 == 1))

    def batch(k, N, ood):
        return make_ood_batch(B, N, seed=9000 + k, paths=paths) if ood else make_batch(B, N, cfg_id=2, seed=9000 + k)

    def check(k, N, w, ood, d, r, rc, tdt):
        nonlocal tot, bad
        f32 = tdt == torch.float32
        tot += B
        if rc is None:
            print("%2d N=%2d %s %s: GPU status %s iters mean %.1f max %d" % (k, N, "ood" if ood else "std", str(tdt)[6:], np.bincount(r["status"], minlength=4).tolist(), r["iters"].mean(), r["iters"].max()), flush=True)
            bad += int((r["status"] == 3).sum())
            return
        p = O.params(N, list(w))
        rel = np.abs(r["cost"] - rc["cost"]) / np.maximum(1.0, np.abs(rc["cost"]))
        both = (r["status"] == 0) & (rc["status"] == 0)
        off = np.where(both & (rel > (1e-3 if f32 else 1e-6)))[0]
        note = ""
        if len(off):
            c = CT.certify_batch(O, p, d, r["U"].astype(np.float64), idx=off, relax=1e-5 if f32 else 1e-8)
            wr = np.maximum(c["ref_scaled_stationarity"], c["ref_scaled_complementarity"])
            unexplained = int((wr > (1e-2 if f32 else 1e-6)).sum())
            note = " other-minimum %d (GPU lower on %d), uncertified %d (worst %.1e)" % (len(off), int((r["cost"][off] < rc["cost"][off]).sum()), unexplained, wr.max())
            bad += unexplained
        print("%2d N=%2d %s %s w=%s: GPU status %s iters mean %.1f max %d | port status %s | max viol %.1e%s" % (k, N, "ood" if ood else "std", str(tdt)[6:], np.array2string(w, precision=2, separator=","),
              np.bincount(r["status"], minlength=4).tolist(), r["iters"].mean(), r["iters"].max(), np.bincount(rc["status"], minlength=4).tolist(), r["viol"].max(), note), flush=True)
        bad += int((r["status"] == 3).sum())

    def port(N, w, d):
        return None if gpu_only else O.solve_condensed_batch(O.params(N, list(w)), d["z0"], d["ref"], d["v_target"], d["u_prev"], nthreads=8)

    if one_launch:
        for N in sorted({st[1] for st in settings}):
            grp = [st for st in settings if st[1] == N]
            ds = [batch(k, N, ood) for k, _, _, ood in grp]
            cat = {q: np.concatenate([d[q] for d in ds]) for q in ("z0", "ref", "v_target", "u_prev")}
            rcs = [port(N, w, d) for (_, _, w, _), d in zip(grp, ds)]
            for tdt in dtypes:
                t0 = time.perf_counter()
                mpc = BatchMPC(N=N, dtype=tdt)
                par = mpc.problem_params(len(grp) * B)
                par[:, BatchMPC.P_WEIGHTS] = torch.as_tensor(np.repeat(np.stack([w for _, _, w, _ in grp]), B, axis=0), dtype=tdt, device=par.device)
                o = mpc.solve(cat["z0"], cat["ref"], cat["v_target"], cat["u_prev"], want_U=True, params=par); torch.cuda.synchronize()
                r = {q: v.cpu().numpy() for q, v in o.items()}
                gpu_s += time.perf_counter() - t0
                mpc.close()
                for j, ((k, _, w, ood), d) in enumerate(zip(grp, ds)):
                    check(k, N, w, ood, d, {q: v[j * B:(j + 1) * B] for q, v in r.items()}, rcs[j], tdt)
    else:
        for k, N, w, ood in settings:
            d = batch(k, N, ood)
            rc = port(N, w, d)
            for tdt in dtypes:
                t0 = time.perf_counter()
                mpc = BatchMPC(N=N, dtype=tdt, weights=list(w))
                o = mpc.solve(d["z0"], d["ref"], d["v_target"], d["u_prev"], want_U=True); torch.cuda.synchronize()
                r = {q: v.cpu().numpy() for q, v in o.items()}
                gpu_s += time.perf_counter() - t0
                mpc.close()
                check(k, N, w, ood, d, r, rc, tdt)
    print("GPU part (%s; handle creation, uploads, solves and downloads; %s): %.3f s" % ("one launch per horizon and precision" if one_launch else "one launch per setting and precision", "fp64" if len(dtypes) == 1 else "both precisions", gpu_s))
    print("problems", tot, "errors or uncertified", bad)


if __name__ == "__main__":
    main()
