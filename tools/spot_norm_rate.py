"""Accuracy and time of the device spot normalisation (sequoia_pub_amd.spotnorm, csrc/spotnorm.hip) beside the numpy / scipy
restatement of the same contract on one core, in ONE process:
    python tools/spot_norm_rate.py [--seconds 0.3] [--rounds 5] [--host_rounds 3] [--out profiles/spot_norm_rate.txt]
First the accuracy over the inputs of tests/test_gpu_spotnorm.py (tests/spotnorm_cases.py: DEVICE_SHAPES): the largest
distance in ulp of the device's l = log1p(x / s) from the extended-precision truth rounded to f64 -- the figure the test's
limit P_DEVICE comes from -- and the largest error over bound of z.
Then the time on one Visium slide: 4992 spots x 33 538 genes, about 3000 expressed genes per spot (about 15 M entries, f32
counts), for 1 gene, 64 genes and all genes, two device paths each, warmed up, then timed in `rounds` windows of about
`seconds` each, the paths alternating, HIP events around each window; the line shows the median window per call and the spread:
    resident     normalize_spots on a CSR matrix in device memory, the result left there
    with copies  upload of data, indices and indptr from pinned memory + the call + download of the result into pinned memory
``read_h5ad`` (libhdf5 and scipy on the host) is timed separately on a file of the same matrix.
The host side is the numpy / scipy restatement of the contract in f64 (tests/spotnorm_cases.py: restate's formulas on the
requested columns) with the BLAS / OpenMP pools limited to one thread where threadpoolctl is installed, `host_rounds` times
between the device's rounds.  IT IS NOT SCANPY: scanpy is not installed here; it works in float32 and in place, and the
reference calls it once per gene.  The yardstick is the project's usual one: a box allows 16 CPUs, so the device path earns
its place where its time with copies is below the host's one-core time / 16.  Prints one line per measurement and a last
JSON line; --out also writes them to a file."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sequoia_pub_amd  # noqa: E402,F401
import spotnorm_cases as sc  # noqa: E402
from sequoia_pub_amd import _lib, spotnorm  # noqa: E402

N_SPOTS, N_GENES, PER_SPOT = 4992, 33538, 3000
HOST_CPUS = 16


def one_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1), "threadpoolctl: 1 thread"
    except ImportError:
        return contextlib.nullcontext(), f"threadpoolctl absent: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"


def window_ms(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def host_restatement(A, cols):
    """The contract in f64 with numpy and scipy for the columns cols (None: all) of the scipy CSR A -> z."""
    F = A.astype(np.float64)
    n = F.shape[0]
    c = np.asarray(F.sum(axis=1)).ravel()
    after = np.median(c[c > 0])
    s = (c + (c == 0)) / after
    dense = (F if cols is None else F[:, cols]).toarray()
    L = np.log1p(dense / s[:, None])
    m = L.sum(axis=0) / n
    d = L - m
    sd = np.sqrt((d * d).sum(axis=0) / (n - 1))
    sd[sd == 0] = 1
    return d / sd


def accuracy(say):
    worst_l, worst_z, where = 0.0, 0.0, None
    for shape in sc.DEVICE_SHAPES:
        n_spots, n_genes, n_empty, full_row = shape
        A = sc.csr_of(sc.counts_case(n_spots, n_genes, 0, n_empty, full_row))
        t = sc.truth_of(n_spots, n_genes, 0, n_empty, full_row)
        csr = spotnorm.csr_to_device(A, "cuda:0")
        L = spotnorm.normalize_spots(*csr, n_genes, scale=False).cpu().numpy()
        z = spotnorm.normalize_spots(*csr, n_genes).cpu().numpy()
        r = sc.restate(A)
        u, uh = sc.ulps(L, t["L"]), sc.ulps(r["L"], t["L"])
        zb = sc.z_bound(n_spots, 2, t)
        live = zb > 0
        ratio = float((np.abs(z - t["z"]).max(axis=0)[live] / zb[live]).max()) if live.any() else 0.0
        say(f"    {n_spots:5d} spots x {n_genes:3d} genes: l {u:.2f} ulp from the rounded truth (numpy on this host: {uh:.2f}); z error / bound(p = 2) {ratio:.3g}")
        if u > worst_l:
            worst_l, where = u, shape
        worst_z = max(worst_z, ratio)
    say(f"log1p on the device: largest distance of l from the rounded truth over the tests' inputs {worst_l:.2f} ulp (at {where}); "
        f"largest z error / bound {worst_z:.3g}")
    return worst_l, worst_z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows_out = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("accuracy over the inputs of tests/test_gpu_spotnorm.py (integer counts):")
    worst_l, worst_z = accuracy(say)

    rs = np.random.default_rng(7)
    mask = rs.random((N_SPOTS, N_GENES), dtype=np.float32) < PER_SPOT / N_GENES
    rows, cols_ = np.nonzero(mask)                               # row-major: every row's indices ascending
    import scipy.sparse as sp
    A = sp.csr_matrix(((1 + rs.poisson(1.5, rows.size)).astype(np.float32), (rows, cols_)), shape=(N_SPOTS, N_GENES))
    A.sort_indices()
    del mask, rows, cols_
    nnz = int(A.nnz)
    say(f"workload: {N_SPOTS} spots x {N_GENES} genes, {nnz} entries ({nnz / N_SPOTS:.0f} per spot), f32 counts")
    pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (A.data, A.indices.astype(np.int32), A.indptr.astype(np.int64))]
    dev = [p.cuda() for p in pinned]
    staged = [torch.empty_like(d) for d in dev]
    limiter, how = one_thread()
    some = np.sort(rs.choice(N_GENES, 64, replace=False))
    for label, cols in (("1 gene", [int(some[0])]), ("64 genes", [int(g) for g in some]), ("all genes", None)):
        C = N_GENES if cols is None else len(cols)
        out_pinned = torch.empty((N_SPOTS, C), dtype=torch.float64).pin_memory()

        def resident():
            return spotnorm.normalize_spots(*dev, N_GENES, cols=cols)

        def with_copies():
            for s_, p in zip(staged, pinned):
                s_.copy_(p, non_blocking=True)
            out_pinned.copy_(spotnorm.normalize_spots(*staged, N_GENES, cols=cols), non_blocking=True)

        paths = {"resident": resident, "with copies": with_copies}
        calls, windows, host_s = {}, {k: [] for k in paths}, []
        for name, fn in paths.items():
            for _ in range(2):
                fn()
            calls[name] = max(2, int(args.seconds * 1e3 / max(window_ms(fn, 2), 1e-3)))
        for r in range(args.rounds):
            for name, fn in paths.items():
                windows[name].append(window_ms(fn, calls[name]))
            if r < args.host_rounds:
                with limiter:
                    t0 = time.perf_counter()
                    zh = host_restatement(A, cols)
                    host_s.append(time.perf_counter() - t0)
                if r == 0:
                    torch.cuda.synchronize()
                    err = float(np.abs(out_pinned.numpy() - zh).max())
                    say(f"{label}: largest |device z - host z| {err:.3g}")
                    assert err < 1e-9, "the device and the host restatement disagree"
                del zh
        med = {k: statistics.median(v) for k, v in windows.items()}
        host_ms = statistics.median(host_s) * 1e3
        say(f"normalize_spots, {label} of {N_SPOTS} x {N_GENES}:")
        for name in windows:
            say(f"    {name:12s} {med[name]:10.4f} ms  (windows {min(windows[name]):.4f}..{max(windows[name]):.4f}, {calls[name]} calls each)")
        met = med["with copies"] < host_ms / HOST_CPUS
        factor = host_ms / HOST_CPUS / med["with copies"]
        say(f"    host, one core (numpy / scipy restatement in f64, NOT scanpy; {how}): {host_ms / 1e3:.3f} s (runs {min(host_s):.3f}..{max(host_s):.3f}); "
            f"/ {HOST_CPUS} CPUs = {host_ms / HOST_CPUS:.1f} ms; with copies {host_ms / med['with copies']:.0f} x one core")
        say(f"    with copies below host / {HOST_CPUS} CPUs: {'met' if met else 'not met'} by a factor of {factor if met else 1 / factor:.1f}")
        rows_out.append(dict(shape=label, resident_ms=round(med["resident"], 5), with_copies_ms=round(med["with copies"], 5),
                             host_s=round(host_ms / 1e3, 4), condition_met=bool(met), factor=round(factor, 2)))
        del out_pinned
        torch.cuda.empty_cache()

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "slide.h5ad")
        from sequoia_pub_amd import h5lite
        with h5lite.File(path, "w") as f:
            g = f.create_group("X")
            g.attrs["encoding-type"] = "csr_matrix"
            g.attrs["shape"] = np.array(A.shape, dtype=np.int64)
            g.create_dataset("data", data=A.data)
            g.create_dataset("indices", data=A.indices.astype(np.int32))
            g.create_dataset("indptr", data=A.indptr.astype(np.int32))
            obs = f.create_group("obs")
            obs.create_dataset("x", data=rs.uniform(0, 20000, N_SPOTS))
            obs.create_dataset("y", data=rs.uniform(0, 20000, N_SPOTS))
            var = f.create_group("var")
            var.attrs["_index"] = "_index"
            var.create_dataset("_index", data=[f"GENE{j}" for j in range(N_GENES)], string="vlen")
        size = os.path.getsize(path)
        reads = []
        for _ in range(3):
            t0 = time.perf_counter()
            m, _, _, names = spotnorm.read_h5ad(path)
            reads.append(time.perf_counter() - t0)
        assert m.nnz == nnz and len(names) == N_GENES
        say(f"read_h5ad of the same matrix ({size / 1e6:.0f} MB, uncompressed CSR, host only): {statistics.median(reads) * 1e3:.0f} ms "
            f"(runs {min(reads) * 1e3:.0f}..{max(reads) * 1e3:.0f})")
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, l_ulp=round(worst_l, 3), z_error_over_bound=round(worst_z, 4),
                        read_h5ad_ms=round(statistics.median(reads) * 1e3, 1), rows=rows_out)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
