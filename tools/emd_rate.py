"""Time of the device earth mover's distance (sequoia_pub_amd.emd, csrc/emd.hip) beside a host solver of the SAME linear
program on one core, in ONE process:
    python tools/emd_rate.py [--sizes 24x25,32x33,50x51,64x64] [--problems 2,128] [--wide_max_cells 2600] [--host_budget 30] [--out profiles/emd_rate.txt]
Workloads: P = 2 and P = 128 problems (64 genes x the raw and the filtered variant is 128) between two maps that fill an
H x W grid -- every cell has weight, as the reference's shifted raw maps have -- at 24 x 25, 32 x 33, 50 x 51 and the cell
limit (64 x 64 = 4096 cells a map).  Two device paths, HIP events around each call, the median of `--repeats` calls after one
warm-up call (a call longer than --long_ms is timed once, and its copies are timed alone and added; a call that ends at a
bound of its work is reported with the library's message):
    resident     emd_grids on grids in device memory, the values left there
    with copies  upload of the grids from pinned memory + the call + download of the P values
The host side is scipy.optimize.linprog(method="highs") -- NOT cv2.EMD, which is not installed here; HiGHS solves the same
transportation problem exactly, cv2 approximates it in float32 -- on ONE problem with the BLAS / OpenMP pools limited to
one thread where threadpoolctl is installed, climbing a ladder of sizes while the power law through the last two solves
predicts the next one within --host_budget seconds.  The device's value is judged by its OWN certificate (value minus
the dual objective u . w_a + v . w_b of the returned plan: zero up to rounding proves the optimum); the relative difference to
HiGHS, which stops at its own tolerances, is printed beside it and not asserted.  Larger
sizes are EXTRAPOLATED with the power law through the two largest sizes timed and marked as such; P problems cost the host P times one.  The yardstick is the project's usual one: a box allows 16 CPUs, so a
device path earns its place where its time with copies is below the host's one-core time / 16.  Prints one line per
measurement and a last JSON line; --out also writes them to a file."""
import argparse
import contextlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, emd  # noqa: E402

HOST_CPUS = 16
HOST_LADDER = [(8, 9), (12, 13), (16, 17), (24, 25), (32, 33), (50, 51), (64, 64)]


def one_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1), "threadpoolctl: 1 thread"
    except ImportError:
        return contextlib.nullcontext(), f"threadpoolctl absent: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"


def maps(P, h, w, seed):
    """P pairs of maps over a full h x w grid: a smooth field plus noise, shifted as get_emd.py:187-188 shifts a raw map."""
    rs = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = []
    for _ in range(2):
        g = np.sin(x * 0.21)[None] + np.cos(y * 0.17)[None] + 0.6 * rs.standard_normal((P, h, w))
        g[:, 0, 0] -= 0.5
        out.append(g + np.abs(g.min(axis=(1, 2), keepdims=True)) + 1e-3)
    return out


def host_lp(arr0, arr1):
    import scipy.sparse as sp
    from scipy.optimize import linprog
    wa, wb = (arr0 / arr0.sum()).ravel(), (arr1 / arr1.sum()).ravel()
    n = wa.size
    xy = np.stack(np.meshgrid(np.arange(arr0.shape[0]), np.arange(arr0.shape[1]), indexing="ij"), -1).reshape(-1, 2)
    d = xy[:, None, :] - xy[None, :, :]
    c = np.sqrt((d[..., 0] ** 2 + d[..., 1] ** 2).astype(np.float64)).ravel()
    a_eq = sp.vstack([sp.kron(sp.identity(n), np.ones((1, n))), sp.kron(np.ones((1, n)), sp.identity(n))]).tocsr()
    t0 = time.perf_counter()
    res = linprog(c, A_eq=a_eq, b_eq=np.concatenate([wa, wb]), bounds=(0, None), method="highs")
    dt = time.perf_counter() - t0
    assert res.status == 0, res.message
    return float(res.fun), dt


def call_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="24x25,32x33,50x51,64x64")
    ap.add_argument("--problems", default="2,128")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--long_ms", type=float, default=1500.0, help="a call longer than this is timed once, not --repeats times")
    ap.add_argument("--wide_max_cells", type=int, default=2600, help="P > 2 is run up to this many cells a map (a wider call above it is minutes to hours)")
    ap.add_argument("--host_budget", type=float, default=30.0, help="the host climbs its ladder of sizes while the next solve is predicted within this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    sizes = [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]
    lines, rows_out = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    # ---- the host: one problem per size, climbing until a solve exceeds the budget
    limiter, how = one_thread()
    host_s = {}
    with limiter:
        for h, w in HOST_LADDER:
            done = sorted(host_s)
            if len(done) >= 2:
                grow = math.log(host_s[done[-1]] / host_s[done[-2]]) / math.log(done[-1] / done[-2])
                if host_s[done[-1]] * (h * w / done[-1]) ** grow > args.host_budget:
                    break
            a0, a1 = maps(1, h, w, 7)
            value, dt = host_lp(a0[0], a1[0])
            vals, plans = emd.emd_grids(torch.from_numpy(a0[0]).cuda(), torch.from_numpy(a1[0]).cuda(), return_plan=True)
            got, pl = float(vals[0]), plans[0]
            gap = got - float((pl["u"] * pl["w_a"]).sum() + (pl["v"] * pl["w_b"]).sum())
            host_s[h * w] = dt
            say(f"host, one core ({how}): linprog/HiGHS on one {h} x {w} problem ({h * w} cells a map, {h * w * h * w} variables): {dt:.2f} s; "
                f"value {value:.12f}, device {got:.12f} (its certificate's gap {gap:.1e}; HiGHS differs by {abs(got - value) / abs(got):.1e} relative)")
    timed = sorted(host_s)
    slope = math.log(host_s[timed[-1]] / host_s[timed[-2]]) / math.log(timed[-1] / timed[-2])
    say(f"host power law through its two largest sizes: seconds ~ cells^{slope:.2f}")

    def host_seconds(cells):
        if cells in host_s:
            return host_s[cells], "timed"
        return host_s[timed[-1]] * (cells / timed[-1]) ** slope, f"EXTRAPOLATED from {timed[-1]} cells with cells^{slope:.2f}"

    for h, w in sizes:
        for P in (int(p) for p in args.problems.split(",")):
            if P > 2 and h * w > args.wide_max_cells:
                say(f"emd_grids: P = {P} problems of {h} x {w} ({h * w} cells a map): NOT RUN (--wide_max_cells {args.wide_max_cells})")
                rows_out.append(dict(shape=f"{h}x{w}", P=P, not_run=True))
                continue
            a0, a1 = maps(P, h, w, 11)
            pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (a0, a1)]
            dev = [t.cuda() for t in pinned]
            staged = [torch.empty_like(t) for t in dev]

            def resident():
                return emd.emd_grids(dev[0], dev[1])

            def with_copies():
                for s, t in zip(staged, pinned):
                    s.copy_(t, non_blocking=True)
                return emd.emd_grids(staged[0], staged[1]).cpu()

            def copies_alone():
                for s, t in zip(staged, pinned):
                    s.copy_(t, non_blocking=True)
                return staged[0][:, 0, 0].contiguous().cpu()

            stats = {}

            def first():                                     # the first timed call also tells the work of problem 0
                _, plans = emd.emd_grids(dev[0], dev[1], return_plan=True)
                stats.update(plans[0], most=max(p["augmentations"] for p in plans), most_steps=max(p["steps"] for p in plans))

            try:
                res = [call_ms(first)]
                if res[0] < args.long_ms:                    # a call of seconds is timed once
                    res = [call_ms(resident) for _ in range(args.repeats)]
                    cop = [call_ms(with_copies) for _ in range(args.repeats)]
                    how_copies = ""
                else:
                    cop = [res[0] + statistics.median(call_ms(copies_alone) for _ in range(3))]
                    how_copies = " (the resident call + the copies timed alone)"
            except RuntimeError as e:
                say(f"emd_grids: P = {P} problems of {h} x {w} ({h * w} cells a map): ENDED at a bound of its work: {e}")
                rows_out.append(dict(shape=f"{h}x{w}", P=P, ended=str(e)))
                continue
            r, c = statistics.median(res), statistics.median(cop)
            one, law = host_seconds(h * w)
            host_ms = one * P * 1e3
            met = c < host_ms / HOST_CPUS
            factor = host_ms / HOST_CPUS / c
            say(f"emd_grids: P = {P} problems of {h} x {w} ({h * w} cells a map; problem 0: {stats['augmentations']} augmentations = {stats['augmentations'] / (2 * h * w):.2f} (n + m), {stats['steps']} search steps; the most of the {P}: {stats['most']} = {stats['most'] / (2 * h * w):.2f} (n + m), {stats['most_steps']} steps)")
            say(f"    resident     {r:12.3f} ms  ({min(res):.3f}..{max(res):.3f}, {len(res)} call{'s' if len(res) > 1 else ''})")
            say(f"    with copies  {c:12.3f} ms  ({min(cop):.3f}..{max(cop):.3f}, {len(cop)} call{'s' if len(cop) > 1 else ''}){how_copies}")
            say(f"    host, one core, linprog/HiGHS: {P} x {one:.2f} s = {host_ms / 1e3:.1f} s ({law}); / {HOST_CPUS} CPUs = {host_ms / HOST_CPUS:.0f} ms")
            say(f"    with copies below host / {HOST_CPUS} CPUs: {'met' if met else 'not met'} by a factor of {factor if met else 1 / factor:.1f}")
            rows_out.append(dict(shape=f"{h}x{w}", P=P, resident_ms=round(r, 3), with_copies_ms=round(c, 3), host_s=round(host_ms / 1e3, 3), host_law=law, augmentations=stats["augmentations"], steps=stats["steps"], most_augmentations=stats["most"], most_steps=stats["most_steps"],
                                 condition_met=bool(met), factor=round(factor, 2)))
            del pinned, dev, staged
    say(json.dumps(dict(repeats=args.repeats, host_solver="scipy.optimize.linprog(method='highs')", rows=rows_out)))


if __name__ == "__main__":
    main()
