"""The k-Means sweep of tests/kmeans_cases.py on the GPU: every case through every entry that admits it, and every output --
labels, seed indices, n_iter, cluster means, the debug entry's final centres -- bit-equal to oracle/kmeans_oracle.py.  No
tolerance anywhere.  The C entries are called directly so that every output can lie between guard elements; the large route also
runs through kmeans_fit(route="large") and the ragged groups through kmeans_fit_ragged, the calls the package makes.
tests/test_kmeans_cases_host.py shows on the CPU that the oracle is scikit-learn's on these cases and that none is marginal."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import kmeans_cases as kc  # noqa: E402
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.kmeans import kmeans_fit, kmeans_fit_ragged, seeding_draws  # noqa: E402

G = kc.GUARD


SENT = {torch.int32: kc.SENT_I32, torch.float32: int(np.array(kc.SENT_F32_BITS, np.uint32).view(np.int32))}


def guarded(numel, dtype):
    """A device buffer of numel elements between two guards; returns (whole buffer as int32, the payload view)."""
    buf = torch.full((numel + 2 * G,), SENT[dtype], dtype=torch.int32, device="cuda")
    return buf, buf[G:G + numel].view(dtype)


def guards_intact(buf, numel, dtype):
    return bool((buf[:G] == SENT[dtype]).all()) and bool((buf[G + numel:] == SENT[dtype]).all())


class Out:
    """The guarded outputs of one call of S slides with `rows` rows in all."""

    def __init__(self, S, rows, k, D, centres=False):
        self.sizes = dict(labels=rows, means=S * k * D, seeds=S * k, n_iter=S)
        if centres:
            self.sizes["centres"] = S * k * D
        self.buf, self.t = {}, {}
        for name, numel in self.sizes.items():
            self.buf[name], self.t[name] = guarded(numel, torch.float32 if name in ("means", "centres") else torch.int32)
        self.S, self.k, self.D = S, k, D

    def ptr(self, name):
        return _lib.ptr(self.t[name])

    def host(self):
        torch.cuda.synchronize()
        for name, numel in self.sizes.items():
            assert guards_intact(self.buf[name], numel, self.t[name].dtype), "guard of " + name
        r = dict(labels=self.t["labels"].cpu().numpy(), cluster_features=self.t["means"].cpu().numpy().reshape(self.S, self.k, self.D),
                 indices=self.t["seeds"].cpu().numpy().reshape(self.S, self.k), n_iter=self.t["n_iter"].cpu().numpy())
        if "centres" in self.t:
            r["centers"] = self.t["centres"].cpu().numpy().reshape(self.S, self.k, self.D)
        return r


def dev(a):
    """A host array (the case module hands them out read-only) as a device tensor."""
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def table_dev(u, k, trials):
    full = np.zeros((max(k - 1, 1), trials), np.float64)         # k = 1: no step reads it, the pointer must still be there
    full[:k - 1] = u[:k - 1]
    return torch.from_numpy(full).cuda()


def c_fit(entry, X, S, n, k, first, u, trials, max_iter=300, tol=1e-4):
    """sq_kmeans_fit (entry "batch", X [S * n, D]) or sq_kmeans_fit_large ("large", S = 1) with guarded outputs."""
    L = _lib.lib()
    D = X.shape[1]
    Xd = dev(X)
    ud = table_dev(u, k, trials)
    need = L.sq_kmeans_workspace_bytes(S, n, D, k) if entry == "batch" else L.sq_kmeans_large_workspace_bytes(n, D, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    o = Out(S, S * n, k, D)
    tail = (_lib.ptr(ud), trials, max_iter, float(tol), o.ptr("labels"), o.ptr("means"), o.ptr("seeds"), o.ptr("n_iter"), _lib.ptr(ws), need,
            _lib.stream_ptr(Xd.device))
    if entry == "batch":
        _lib.check(L.sq_kmeans_fit(_lib.ptr(Xd), S, n, D, k, first, *tail))
    else:
        _lib.check(L.sq_kmeans_fit_large(_lib.ptr(Xd), n, D, k, first, *tail))
    return o.host()


def same_means(got, want):
    """Bit equality of the cluster means, NaN rows where the oracle has them (and nowhere else)."""
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)


def check_fit(got, s, lo, hi, ref, what):
    assert np.array_equal(got["indices"][s], ref["indices"]), (what, "seed indices")
    assert int(got["n_iter"][s]) == ref["n_iter"], (what, "n_iter", int(got["n_iter"][s]), ref["n_iter"])
    assert np.array_equal(got["labels"][lo:hi], ref["labels"]), (what, "labels", int((got["labels"][lo:hi] != ref["labels"]).sum()))
    assert same_means(got["cluster_features"][s], ref["cluster_means"]), (what, "cluster means")


GRAM_ROWS = [r for r in kc.ROWS if r.n <= kc.GRAM_MAX_N]


@pytest.mark.parametrize("row", GRAM_ROWS, ids=lambda r: r.name)
def test_rows_through_sq_kmeans_fit(row):
    _lib.require_gpu()
    first, u = seeding_draws(row.n, row.k, 0)
    got = c_fit("batch", kc.row_data(row), 1, row.n, row.k, first, u, kc.trials_of(row.k))
    check_fit(got, 0, 0, row.n, kc.row_reference(row), row.name)


@pytest.mark.parametrize("row", kc.ROWS, ids=lambda r: r.name)
def test_rows_through_the_large_route(row):
    _lib.require_gpu()
    assert row.n <= kc.LARGE_MAX_N
    r = kmeans_fit(dev(kc.row_data(row)), row.k, route="large")
    got = dict(labels=r["labels"][0].cpu().numpy(), indices=r["indices"].cpu().numpy(), n_iter=r["n_iter"].cpu().numpy(),
               cluster_features=r["cluster_features"].cpu().numpy())
    check_fit(got, 0, 0, row.n, kc.row_reference(row), row.name)
    first, u = seeding_draws(row.n, row.k, 0)                    # and the entry itself, between guards
    check_fit(c_fit("large", kc.row_data(row), 1, row.n, row.k, first, u, kc.trials_of(row.k)), 0, 0, row.n, kc.row_reference(row), row.name)


@pytest.mark.parametrize("group", kc.ragged_groups(), ids=lambda g: "+".join(r.name for r in g))
def test_rows_sharing_dim_and_k_in_one_ragged_call(group):
    _lib.require_gpu()
    L = _lib.lib()
    k, D = group[0].k, group[0].dim
    counts = np.array([r.n for r in group], np.int32)
    firsts = np.array([seeding_draws(r.n, k, 0)[0] for r in group], np.int32)
    X = dev(np.concatenate([kc.row_data(r) for r in group]))
    ud = table_dev(seeding_draws(k, k, 0)[1], k, kc.trials_of(k))
    need = int(L.sq_kmeans_ragged_workspace_bytes(len(group), counts.ctypes.data, D, k))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    o = Out(len(group), int(counts.sum()), k, D)
    _lib.check(L.sq_kmeans_fit_ragged(_lib.ptr(X), len(group), counts.ctypes.data, D, k, firsts.ctypes.data, _lib.ptr(ud), kc.trials_of(k), 300, 1e-4,
                                      o.ptr("labels"), o.ptr("means"), o.ptr("seeds"), o.ptr("n_iter"), _lib.ptr(ws), need, _lib.stream_ptr(X.device)))
    got = o.host()
    lo = 0
    for s, r in enumerate(group):
        check_fit(got, s, lo, lo + r.n, kc.row_reference(r), r.name)
        lo += r.n
    # the same group through the package's call
    p = kmeans_fit_ragged([dev(kc.row_data(r)) for r in group], k)
    for s, r in enumerate(group):
        ref = kc.row_reference(r)
        assert np.array_equal(p["labels"][s].cpu().numpy(), ref["labels"]) and np.array_equal(p["indices"][s].cpu().numpy(), ref["indices"]), r.name
        assert int(p["n_iter"][s]) == ref["n_iter"] and same_means(p["cluster_features"][s].cpu().numpy(), ref["cluster_means"]), r.name


@pytest.mark.parametrize("entry", ["batch", "large"])
@pytest.mark.parametrize("trow", kc.TRIAL_ROWS, ids=lambda t: t.name)
def test_one_and_eight_trials(trow, entry):
    _lib.require_gpu()
    X = kc.data(trow.kind, trow.seed, trow.n, trow.dim)
    got = c_fit(entry, X, 1, trow.n, trow.k, trow.first, kc.trial_table(trow.k, trow.trials), trow.trials)
    check_fit(got, 0, 0, trow.n, kc.trial_reference(trow.name), (trow.name, entry))


@pytest.mark.parametrize("entry", ["batch", "large"])
@pytest.mark.parametrize("case", kc.STOP_CASES, ids=lambda c: c.name)
def test_stop_rules(case, entry):
    _lib.require_gpu()
    row = kc.ROW[kc.STOP_ROW]
    first, u = seeding_draws(row.n, row.k, 0)
    got = c_fit(entry, kc.row_data(row), 1, row.n, row.k, first, u, kc.trials_of(row.k), case.max_iter, case.tol)
    ref = kc.row_reference(row, case.max_iter, case.tol)
    check_fit(got, 0, 0, row.n, ref, (case.name, entry))
    if case.max_iter == 0:
        assert int(got["n_iter"][0]) == 0                        # no iteration; the labels are the E-step against the seeds


def test_three_slides_that_stop_for_different_reasons():
    """One sq_kmeans_fit call: two slides converge strictly inside a burst, one runs into max_iter -- the closing E-step is
    forced for all three and the strict slides' labels are put back."""
    _lib.require_gpu()
    b = kc.BATCH_STOP
    X = np.concatenate([kc.data(kind, seed, b.n, b.dim) for kind, seed in zip(b.kinds, b.seeds)])
    first, u = seeding_draws(b.n, b.k, 0)
    got = c_fit("batch", X, 3, b.n, b.k, first, u, kc.trials_of(b.k), b.max_iter)
    refs = [kc.fit_reference(kind, seed, b.n, b.dim, b.k, b.max_iter) for kind, seed in zip(b.kinds, b.seeds)]
    assert {r["trace"]["strict"] for r in refs} == {True, False}
    for s, ref in enumerate(refs):
        check_fit(got, s, s * b.n, (s + 1) * b.n, ref, s)


DBG_PARAMS = [(d.name, large) for d in kc.DBG_ROWS for large in ((0, 1) if kc.dbg_inputs(d.name)[0].shape[0] == 1 else (0,))]


@pytest.mark.parametrize("name,large_lists", DBG_PARAMS, ids=lambda v: str(v))
def test_lloyd_from_given_centres(name, large_lists):
    """sq_dbg_kmeans_lloyd against ko.lloyd on ko.center_data(X): labels, n_iter, cluster means and the final centres (both
    sum a cluster's members in index order in fp64), with the member lists of either route."""
    _lib.require_gpu()
    L = _lib.lib()
    d = kc.DBG[name]
    X, C = kc.dbg_inputs(name)
    S, n, D = X.shape
    k = C.shape[1]
    Xd, Cd = dev(X.reshape(S * n, D)), dev(C)
    need = L.sq_kmeans_workspace_bytes(S, n, D, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    o = Out(S, S * n, k, D, centres=True)
    _lib.check(L.sq_dbg_kmeans_lloyd(_lib.ptr(Xd), S, n, D, k, _lib.ptr(Cd), large_lists, d.max_iter, float(d.tol), o.ptr("labels"), o.ptr("means"),
                                     o.ptr("centres"), o.ptr("n_iter"), _lib.ptr(ws), need, _lib.stream_ptr(Xd.device)))
    got = o.host()
    ref = kc.dbg_reference(name)
    assert np.array_equal(got["n_iter"], ref["n_iter"]), (got["n_iter"], ref["n_iter"])
    assert np.array_equal(got["labels"].reshape(S, n), ref["labels"])
    assert np.array_equal(got["centers"].view(np.int32), ref["centers"].view(np.int32))          # bit patterns
    for s in range(S):
        assert same_means(got["cluster_features"][s], ref["cluster_means"][s]), s
    assert bool((o.t["seeds"] == kc.SENT_I32).all())             # the entry writes no seed indices (none were handed to it)


def test_refusals_name_their_bound_and_a_fit_still_works():
    _lib.require_gpu()
    L = _lib.lib()
    ns, fc = np.array([300], np.int32), np.zeros(1, np.int32)

    def refused(n, D, k, trials, needle):
        calls = [L.sq_kmeans_fit(None, 1, n, D, k, 0, None, trials, 300, 1e-4, None, None, None, None, None, 0, None),
                 L.sq_kmeans_fit_large(None, n, D, k, 0, None, trials, 300, 1e-4, None, None, None, None, None, 0, None)]
        for i, rc in enumerate(calls):                           # NULL data and no workspace: nothing can have been launched
            assert rc != 0 and needle in L.sq_last_error(), (i, needle, L.sq_last_error())
        ns[0] = n
        rc = L.sq_kmeans_fit_ragged(None, 1, ns.ctypes.data, D, k, fc.ctypes.data, None, trials, 300, 1e-4, None, None, None, None, None, 0, None)
        assert rc != 0 and needle in L.sq_last_error(), (needle, L.sq_last_error())
        if trials == 6:                                          # the debug entry has no trial count
            rc = L.sq_dbg_kmeans_lloyd(None, 1, n, D, k, None, 0, 300, 1e-4, None, None, None, None, None, 0, None)
            assert rc != 0 and needle in L.sq_last_error(), (needle, L.sq_last_error())

    refused(300, 64, 0, 6, b"n_clusters=0, must be in 1..256")
    refused(300, 64, 257, 6, b"n_clusters=257, must be in 1..256")
    refused(300, 6, 8, 6, b"dim=6 must be a multiple of 4")
    refused(300, 64, 8, 0, b"n_local_trials=0, must be in 1..8")
    refused(300, 64, 8, 9, b"n_local_trials=9, must be in 1..8")
    refused(5, 64, 8, 6, b"n_samples=5, must be in n_clusters=8..")
    assert L.sq_kmeans_workspace_bytes(1, 300, 64, 0) == 0 and L.sq_kmeans_large_workspace_bytes(300, 64, 0) == 0
    rc = L.sq_dbg_kmeans_lloyd(None, 2, 300, 64, 8, None, 1, 300, 1e-4, None, None, None, None, None, 0, None)
    assert rc != 0 and b"null pointer" in L.sq_last_error()      # the pointers come before the one-slide rule of large_lists
    row = kc.ROW["k8_dim36"]                                     # a valid fit afterwards still works
    first, u = seeding_draws(row.n, row.k, 0)
    check_fit(c_fit("batch", kc.row_data(row), 1, row.n, row.k, first, u, kc.trials_of(row.k)), 0, 0, row.n, kc.row_reference(row), "after refusals")
