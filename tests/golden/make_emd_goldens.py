#!/usr/bin/env python3
"""Writes tests/golden/emd_fastemd.npz: histograms and the values the reference's own solver gives for them.

    python tests/golden/make_emd_goldens.py --reference <checkout of the reference>

Needs g++ and the reference's code_for_Metrics/FastEMD headers; run where both exist, not by the test suite.  The script writes a
small driver of its own into a temporary directory, compiles it against those headers and feeds it every case: the driver
builds D as EMD.m does (Euclidean distance of the bin centres of an R x C grid, bins in row-major order) and calls
emd_hat_gd_metric<double, NO_FLOW>(P, Q, D, 0).  Only data is kept: the inputs, the scores as printed with %.17g, and the
solver's CPU time per case (one core; the figure DESIGN.md quotes beside the device's)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

DRIVER = r"""
#include <cstddef>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <ctime>
#include <vector>
#include "emd_hat.hpp"
int main() {
  int R, C;
  while (scanf("%d %d", &R, &C) == 2) {
    const int N = R * C;
    std::vector<double> P(N), Q(N);
    for (int i = 0; i < N; ++i) if (scanf("%lf", &P[i]) != 1) return 1;
    for (int i = 0; i < N; ++i) if (scanf("%lf", &Q[i]) != 1) return 1;
    std::vector<std::vector<double> > D(N, std::vector<double>(N));
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        const double dr = i / C - j / C, dc = i % C - j % C;
        D[i][j] = sqrt(dr * dr + dc * dc);
      }
    const clock_t t0 = clock();
    const double v = emd_hat_gd_metric<double, NO_FLOW>()(P, Q, D, 0);
    printf("%.17g %.6f\n", v, (double)(clock() - t0) / CLOCKS_PER_SEC);
  }
  return 0;
}
"""


def cases():
    """-> [(name, R, C, P, Q)]"""
    rng = np.random.default_rng(20240611)
    out = []

    def norm(v, total=1.0):
        return v * (total / v.sum())

    def dense(n):
        return norm(rng.random(n) + 0.01)

    def sparse(n, empty):
        v = rng.random(n) * (rng.random(n) >= empty)
        if not v.any():
            v[rng.integers(n)] = 1.0
        return norm(v)

    def point(n, i):
        v = np.zeros(n)
        v[i] = 1.0
        return v

    for R, C in ((1, 2), (1, 3), (2, 2), (2, 3)):
        out.append(("dense_%dx%d" % (R, C), R, C, dense(R * C), dense(R * C)))
    out.append(("dense_5x13", 5, 13, dense(65), dense(65)))
    out.append(("dense_7x12", 7, 12, dense(84), dense(84)))
    out.append(("dense_12x20", 12, 20, dense(240), dense(240)))
    out.append(("empty30_7x12", 7, 12, sparse(84, 0.3), sparse(84, 0.3)))
    out.append(("empty60_5x13", 5, 13, sparse(65, 0.6), sparse(65, 0.6)))
    out.append(("empty90_12x20", 12, 20, sparse(240, 0.9), sparse(240, 0.9)))
    out.append(("one_source_7x12", 7, 12, point(84, 40), dense(84)))
    out.append(("one_sink_7x12", 7, 12, dense(84), point(84, 13)))
    q = sparse(65, 0.3)
    out.append(("equal_5x13", 5, 13, q.copy(), q.copy()))
    q = dense(84)
    out.append(("permutation_7x12", 7, 12, q[rng.permutation(84)], q))
    for k, (R, C) in enumerate(((2, 3), (7, 12))):
        # a few negative bins on either side, as bicubic resizing leaves them: they pin the pre-flow rule
        p, q = rng.random(R * C) + 0.01, rng.random(R * C) + 0.01
        p[rng.choice(R * C, 2, replace=False)] = -0.05
        q[rng.choice(R * C, 1 + k, replace=False)] = -0.03
        out.append(("negative_%dx%d" % (R, C), R, C, norm(p), norm(q)))
    out.append(("unequal_sums_5x13", 5, 13, dense(65), norm(dense(65), 0.9)))
    out.append(("unequal_sums_swapped_2x3", 2, 3, norm(dense(6), 0.8), dense(6)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's checkout (holds code_for_Metrics/FastEMD)")
    ap.add_argument("--out", default=os.path.join(HERE, "emd_fastemd.npz"))
    args = ap.parse_args()
    inc = os.path.join(args.reference, "code_for_Metrics", "FastEMD")
    assert os.path.exists(os.path.join(inc, "emd_hat.hpp")), "no emd_hat.hpp under %s" % inc
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["g++", "-O2", "-w", "-I", inc, src, "-o", exe], check=True)
        text = "".join("%d %d\n%s\n%s\n" % (R, C, " ".join("%.17g" % v for v in P), " ".join("%.17g" % v for v in Q))
                       for _, R, C, P, Q in cs)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    arrays, meta = {}, []
    for (name, R, C, P, Q), line in zip(cs, lines):
        score, secs = line.split()
        arrays[name + "_P"], arrays[name + "_Q"] = P, Q
        meta.append(dict(name=name, R=R, C=C, score=score, cpu_seconds=float(secs)))
        print(name, R, C, score, secs)
    assert len(meta) == len(cs)
    np.savez_compressed(args.out, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    sys.exit(main())
