"""Record what the reference's own PidControl and LowPass classes compute -> tests/golden/lowlevel_classes.npz (arrays only).

The two classes behind the reference's low-level controller (src/PidControl.h, src/LowPass.h) are header-only C++ without ROS.  This tool writes a
small driver of its own into a temporary directory, compiles it against the reference's headers (g++ -O2 -ffp-contract=off -I REFERENCE/src), runs
it on seeded inputs and stores inputs and outputs.  Nothing of the reference's text and no binary is kept: the temporary directory is removed.
The callback that composes the two classes (LowLevelController.cpp) needs ROS to compile; it is restated by reading (include/kmpc.h).

The inputs lie on binary grids so that the device kernel can be fed them exactly through its own arithmetic (tests/test_lowlevel.py):
  lp_in    400 values 50 * v with v a multiple of 2^-30, |v| < 1: raw = 50.0 * (v - 0) is lp_in exactly
  pid_err  400 errors, multiples of 2^-40 inside (-3.5, 3.5): ac = 12.5 + e and e = ac - 12.5 are both exact
  pid_reset  the indices before whose step resetIntegrator() was called

usage: python tools/make_lowlevel_fixture.py REFERENCE_DIR [-o tests/golden/lowlevel_classes.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

SEED, N = 20261019, 400
TAU, TS = 0.5, 0.02                    # lpf_accel_.setParams(0.5, 0.02)
KP, KI, KD, LO, HI, DT = 0.8, 0.4, 0.0, 0.0, 1.0, 0.02

DRIVER = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "PidControl.h"
#include "LowPass.h"
using namespace dbw_mkz_low_level_controller;
// stdin: int64 n, n doubles (low-pass inputs), n doubles (pid errors), n doubles (1.0 = resetIntegrator() before this step)
// stdout: n doubles LowPass(tau, ts).filt, n doubles PidControl(kp, ki, kd, lo, hi).step(e, dt)
int main(int argc, char **argv)
{
    if (argc != 9) return 2;
    const double tau = atof(argv[1]), ts = atof(argv[2]), kp = atof(argv[3]), ki = atof(argv[4]), kd = atof(argv[5]), lo = atof(argv[6]),
                 hi = atof(argv[7]), dt = atof(argv[8]);
    long long n = 0;
    if (fread(&n, sizeof n, 1, stdin) != 1 || n < 1 || n > 1000000) return 3;
    std::vector<double> in(3 * n), out(2 * n);
    if (fread(in.data(), sizeof(double), 3 * n, stdin) != (size_t)(3 * n)) return 4;
    LowPass lp(tau, ts);
    for (long long k = 0; k < n; ++k) out[k] = lp.filt(in[k]);
    PidControl pid;
    pid.setGains(kp, ki, kd);
    pid.setRange(lo, hi);
    for (long long k = 0; k < n; ++k) {
        if (in[2 * n + k] != 0.0) pid.resetIntegrator();
        out[n + k] = pid.step(in[n + k], dt);
    }
    return fwrite(out.data(), sizeof(double), 2 * n, stdout) == (size_t)(2 * n) ? 0 : 5;
}
"""


def inputs():
    rng = np.random.default_rng(SEED)
    v = np.clip(np.cumsum(rng.normal(0.0, 0.01, N)) + rng.normal(0.0, 0.005, N), -0.9, 0.9)
    v = np.round(v * 2.0 ** 30) / 2.0 ** 30
    lp_in = 50.0 * v                                                  # exact: 6 bits x at most 30
    err = np.clip(rng.normal(0.3, 0.9, N) + 0.8 * np.sin(np.arange(N) / 25.0), -3.4, 3.4)
    err = np.round(err * 2.0 ** 40) / 2.0 ** 40
    reset = np.zeros(N)
    reset[np.sort(rng.choice(np.arange(5, N), 9, replace=False))] = 1.0
    assert (lp_in / 50.0 == v).all() and ((12.5 + err) - 12.5 == err).all() and (err != 0.0).all()
    return lp_in, err, reset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "lowlevel_classes.npz"))
    a = ap.parse_args()
    src = os.path.join(a.reference, "src")
    for h in ("PidControl.h", "LowPass.h"):
        if not os.path.exists(os.path.join(src, h)):
            sys.exit("%s not found under %s" % (h, src))
    lp_in, err, reset = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.cpp"), "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", src, "-o", exe, os.path.join(tmp, "driver.cpp")])
        blob = np.int64(N).tobytes() + np.concatenate([lp_in, err, reset]).astype(np.float64).tobytes()
        out = subprocess.run([exe] + [repr(x) for x in (TAU, TS, KP, KI, KD, LO, HI, DT)], input=blob, stdout=subprocess.PIPE, check=True).stdout
    out = np.frombuffer(out, dtype=np.float64)
    assert out.shape == (2 * N,)
    lp_out, pid_out = out[:N].copy(), out[N:].copy()
    assert (pid_out == 1.0).sum() >= 10 and (pid_out == 0.0).sum() >= 10 and ((pid_out > 0.0) & (pid_out < 1.0)).sum() >= 100   # clips at both ends
    np.savez(a.out, lp_in=lp_in, lp_out=lp_out, lp_params=np.array([TAU, TS]), pid_err=err, pid_out=pid_out,
             pid_reset=np.flatnonzero(reset).astype(np.int64), pid_params=np.array([KP, KI, KD, LO, HI, DT]))
    print("%s: %d low-pass values, %d PID steps (%d at the upper limit, %d at the lower, %d resets), %d bytes"
          % (a.out, N, N, (pid_out == 1.0).sum(), (pid_out == 0.0).sum(), int(reset.sum()), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
