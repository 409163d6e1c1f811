"""Rate of the two feeds of the training loops, the DataLoader path beside the device-resident path, in ONE process:
    python tools/train_feed_rate.py [--slides 2048] [--dim 1024] [--genes 20820] [--epochs 5] [--out profiles/train_feed_rate.txt]
A synthetic cohort (synth.cluster_tokens, synth.rna_targets) is written as one store file per slide into a temporary directory.
Measured:
 (a) the one-off cost of the resident feed: CohortTable (every store read once, serially) and its upload, host clock, seconds.
 (b) sq_cohort_gather alone at B = 16 and B = 64 on random rows of the uploaded tables, beside torch.index_select of the same rows
     (two calls: features, targets): --repeats launches between two device events, queued while the device is still busy with
     --blocker matrix products (so the device's time is measured, not the host's launch rate; the tool stops if the device caught
     up), windows alternating between the two, median and range over --windows windows; microseconds per batch and TB/s of
     bytes read plus written, B * (tokens * D + G) * 4 * 2; beside it the host's time to queue one batch.
     The tables (1 GB at the default size) exceed the 256 MB last-level cache, the outputs (26 MB at B = 64) do not.
 (c) one training epoch of ViS (depth 6, 16 heads, bf16, batch 64) through train() and of HE2RNA (fused engine, batch 16) through
     fit(), with each feed.  ONE call of train() / fit() runs all epochs on one model; the loader it is given hands out the two
     feeds in turn, a whole epoch each, and stamps the host clock after a device synchronise at every epoch boundary.  The first
     epoch of each feed is warm-up; reported: median and range of the next --epochs epochs of each feed, the ratio of the medians
     and "resident not slower than loader: met / not met" (met: the resident median is not above the loader median).  Both feeds
     keep the per-batch statistics download of train().
Every GPU step runs under a time limit of its own: SIGALRM with its default action ends the process when a step overruns.
Prints one line per measurement and a last JSON line; --out also writes them to a file."""
import argparse
import json
import os
import signal
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, store, synth  # noqa: E402
from sequoia_pub_amd import he2rna as he  # noqa: E402
from sequoia_pub_amd.data import CohortTable, ResidentLoader, SuperTileRNADataset, cohort_gather, custom_collate_fn  # noqa: E402
from sequoia_pub_amd.train import train  # noqa: E402
from sequoia_pub_amd.vis import ViS  # noqa: E402

COPY_TBS = 6.29          # MI355X float4 copy, bytes read plus written
PROJECT = "TCGA-SYN"


class step_limit:
    """`with step_limit(seconds):` -- the process is ended by SIGALRM if the block takes longer (also inside a C call)."""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def write_cohort(root, slides, tokens, dim, genes, chunk=256):
    """One store per slide under root/PROJECT; returns the reference frame (the targets as its rna_ columns)."""
    rows = []
    for lo in range(0, slides, chunk):
        x = synth.cluster_tokens(100 + lo, min(chunk, slides - lo), dim, tokens)
        for i in range(x.shape[0]):
            name = f"SYN-{lo + i:05d}"
            d = os.path.join(root, PROJECT, name)
            os.makedirs(d)
            with store.File(os.path.join(d, name + ".h5"), "w") as f:
                f.create_dataset("cluster_features", data=x[i])
            rows.append(name)
    frame = pd.DataFrame(synth.rna_targets(7, slides, genes), columns=[f"rna_G{g}" for g in range(genes)])
    frame.insert(0, "tcga_project", PROJECT)
    frame.insert(0, "patient_id", rows)
    frame.insert(0, "wsi_file_name", rows)
    return frame


class AlternatingFeed:
    """The loader train() / fit() is given: epoch e is a whole pass of feeds[e % 2]; a host-clock stamp, after a device
    synchronise, at the start of every epoch (and one from close())."""
    sampler = None

    def __init__(self, feeds):
        self.feeds, self.stamps = feeds, []

    def _stamp(self):
        torch.cuda.synchronize()
        self.stamps.append(time.perf_counter())

    def __iter__(self):
        loader = self.feeds[(len(self.stamps)) % len(self.feeds)][1]
        self._stamp()
        return iter(loader)

    def __len__(self):
        return len(self.feeds[0][1])

    def close(self):
        """Seconds per epoch and feed, the first epoch of each feed (warm-up) left out."""
        self._stamp()
        spans = np.diff(self.stamps)
        return {name: [float(s) for s in spans[i::len(self.feeds)][1:]] for i, (name, _) in enumerate(self.feeds)}


def gather_windows(table, B, repeats, windows, blocker, dev):
    """Microseconds per batch of sq_cohort_gather and of torch.index_select on the same random rows, per window: (device, host enqueue).
    A window's launches are queued while the device still works on `blocker` large matrix products, so the time between the two
    events around them is the device's, back to back, and not the host's rate of launching."""
    g = torch.Generator().manual_seed(B)
    rows = [torch.randint(0, len(table), (B,), generator=g) for _ in range(repeats)]
    idx32, idx64 = [r.to(torch.int32).to(dev) for r in rows], [r.to(dev) for r in rows]
    x_out, y_out = (torch.empty((B,) + tuple(t.shape[1:]), device=dev) for t in (table.x_dev, table.y_dev))

    def ours(i):
        cohort_gather(table.x_dev, idx32[i], table.y_dev, x_out=x_out, y_out=y_out)

    def torchs(i):
        torch.index_select(table.x_dev, 0, idx64[i], out=x_out)
        torch.index_select(table.y_dev, 0, idx64[i], out=y_out)

    ours(0)
    mine = (x_out.clone(), y_out.clone())
    torchs(0)
    assert torch.equal(mine[0], x_out) and torch.equal(mine[1], y_out), "sq_cohort_gather and torch.index_select disagree"
    big = torch.randn(8192, 8192, device=dev)
    res = {"sq_cohort_gather": [], "torch.index_select": []}
    enqueue = {"sq_cohort_gather": [], "torch.index_select": []}
    for _ in range(windows):
        for name, fn in (("sq_cohort_gather", ours), ("torch.index_select", torchs)):
            busy, start, end = torch.cuda.Event(), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            for _ in range(blocker):
                big @ big                                              # the device is busy while the launches are queued behind it
            busy.record()
            start.record()
            t0 = time.perf_counter()
            for i in range(repeats):
                fn(i)
            enqueue[name].append((time.perf_counter() - t0) * 1e6 / repeats)
            end.record()
            if busy.query():
                raise SystemExit(f"{name}: the device caught up with the host while {repeats} launches were queued: raise --blocker")
            end.synchronize()
            res[name].append(start.elapsed_time(end) * 1e3 / repeats)
    return res, enqueue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slides", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--genes", type=int, default=20820)
    ap.add_argument("--epochs", type=int, default=5, help="timed epochs per feed (one more each is warm-up)")
    ap.add_argument("--repeats", type=int, default=200, help="gather launches per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--blocker", type=int, default=8, help="8192^3 f32 matrix products in front of a gather window")
    ap.add_argument("--limit", type=int, default=600, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    dev = "cuda:0"
    lines, result = [], {}

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        frame = write_cohort(root, args.slides, args.tokens, args.dim, args.genes)
        say(f"cohort: {args.slides} slides x {args.tokens} tokens x {args.dim} f32, {args.genes} genes, one store per slide "
            f"({store.backend()} backend), written in {time.perf_counter() - t0:.1f} s")

        # ---- (a) the one-off load and upload
        with step_limit(args.limit):
            torch.zeros(1, device=dev)                                 # the device context is not part of the upload
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = CohortTable(frame, root)
            t1 = time.perf_counter()
            table.to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        result["load_s"], result["upload_s"], result["table_bytes"] = t1 - t0, t2 - t1, table.nbytes
        say(f"(a) resident feed, once per run: {args.slides} stores read in {t1 - t0:.2f} s ({(t1 - t0) / args.slides * 1e3:.2f} ms per slide), "
            f"{table.nbytes / 1e9:.2f} GB uploaded through one pinned buffer in {t2 - t1:.2f} s ({table.nbytes / 1e9 / (t2 - t1):.1f} GB/s)")

        # ---- (b) the gather alone
        result["gather_us"], result["gather_enqueue_us"] = {}, {}
        for B in (16, 64):
            with step_limit(args.limit):
                res, enqueue = gather_windows(table, B, args.repeats, args.windows, args.blocker, dev)
            moved = B * (args.tokens * args.dim + args.genes) * 4 * 2
            result["gather_us"][B], result["gather_enqueue_us"][B] = res, enqueue
            say(f"(b) one batch of {B} slides ({moved / 1e6:.1f} MB read plus written), {args.repeats} launches per window, {args.windows} windows:")
            for name, us in res.items():
                med = statistics.median(us)
                say(f"    {name:18s} median {med:8.2f} us ({min(us):.2f}..{max(us):.2f}) = {moved / med / 1e6:.2f} TB/s "
                    f"({moved / med / 1e6 / COPY_TBS * 100:.0f} % of the {COPY_TBS} TB/s float4 copy); the host queues one in "
                    f"{statistics.median(enqueue[name]):.1f} us")

        # ---- (c) whole epochs through train() and fit()
        rows = np.arange(args.slides)
        epochs = 2 * (args.epochs + 1)

        def feeds(batch):
            dataset = SuperTileRNADataset(frame, root)
            return AlternatingFeed([
                ("loader", DataLoader(dataset, num_workers=0, pin_memory=True, shuffle=True, batch_size=batch, collate_fn=custom_collate_fn)),
                ("resident", ResidentLoader(table, rows, batch, shuffle=True))])

        result["epoch_s"] = {}
        for model_name, batch in (("ViS depth 6, 16 heads, bf16", 64), ("HE2RNA fused", 16)):
            torch.manual_seed(0)
            np.random.seed(0)
            feed = feeds(batch)
            with step_limit(args.limit):
                if model_name.startswith("ViS"):
                    model = ViS(num_outputs=args.genes, input_dim=args.dim, depth=6, nheads=16, dimensions_f=64, dimensions_c=64,
                                dimensions_s=64, device=dev, compute_dtype="bf16").to(dev)
                    train(model, {"train": feed}, None, num_epochs=epochs, phases=["train"], save_dir=None, verbose=False, patience=epochs + 1)
                else:
                    model = he.HE2RNA(input_dim=args.dim, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], output_dim=args.genes, device=dev)
                    he.fit(model=model, lr=1e-3, train_loader=feed, valid_loader=None, test_loader=None, params={"max_epochs": epochs},
                           path=None, verbose=False, engine="fused", seed=0)
                spans = feed.close()
            del model
            result["epoch_s"][model_name] = spans
            med = {k: statistics.median(v) for k, v in spans.items()}
            say(f"(c) {model_name}, batch {batch}: one epoch of {args.slides} slides ({len(feed)} steps), {args.epochs} epochs per feed, alternating:")
            for k, v in spans.items():
                say(f"    {k:8s} median {med[k]:8.3f} s per epoch ({min(v):.3f}..{max(v):.3f}) = {med[k] / len(feed) * 1e3:8.2f} ms per step")
            met = med["resident"] <= med["loader"]
            say(f"    loader / resident = {med['loader'] / med['resident']:.2f}; resident not slower than loader: {'met' if met else 'not met'}")
            result.setdefault("not_slower", {})[model_name] = bool(met)
    say(json.dumps(result))


if __name__ == "__main__":
    main()
