"""KMeans -- host-side mirror of the interface /root/reference/pre_processing/kmean_features.py:96-97
uses (``sklearn.cluster.KMeans(n_clusters, random_state=0).fit(X).labels_``) plus the cluster-mean
step of :99-108, on the HIP k-means kernels (``sq_kmeans_fit``; ``sq_kmeans_fit_large`` for slides of more
than ``GRAM_MAX_ROWS`` patches, which a raised ``--max_patch_number`` produces: compute_features_hdf5.py:26,112-113).
``kmeans_fit_ragged`` is the loop over slides around it (kmean_features.py:65-108): slides of different patch counts in one
``sq_kmeans_fit_ragged`` call, every slide bit-equal to its own ``kmeans_fit``.

The only host arithmetic is the data-independent MT19937 draw sequence of scikit-learn's
``_kmeans_plusplus`` (``RandomState(random_state).choice(n, p=uniform)`` then ``uniform(size=2+log k)``
per further centre), produced here with numpy's ``RandomState`` and handed to the kernel."""
import numpy as np
import torch

from . import _abi, _lib


def seeding_draws(n_samples, n_clusters, random_state=0):
    """sklearn/cluster/_kmeans.py:222-243: (first_center, uniforms[k-1, 2+int(log k)])."""
    rs = np.random.RandomState(random_state)
    sw = np.ones(n_samples, dtype=np.float32)
    first = int(rs.choice(n_samples, p=sw / sw.sum()))
    trials = 2 + int(np.log(n_clusters))
    u = np.empty((max(n_clusters - 1, 1), trials), dtype=np.float64)
    for c in range(n_clusters - 1):
        u[c] = rs.uniform(size=trials)
    return first, u


GRAM_MAX_ROWS = 4096          # sq_kmeans_fit seeds from one n x n Gram matrix per slide and stops here
LARGE_MAX_ROWS = _abi.CONSTANTS["SQ_KMEANS_LARGE_MAX_SAMPLES"]       # the bound of sq_kmeans_fit_large
RAGGED_MAX_SLIDES = 4096      # slides per sq_kmeans_fit_ragged call

_uniforms_cache = {}          # (k, seed, device) -> (device table, trials)
_first_cache = {}             # (n, k, seed) -> first centre


def _uniforms(n_clusters, random_state, dev):
    """The uniforms of seeding_draws on the device.  They do not depend on the patch count, and the reference clusters
    every slide with the same ``random_state`` (kmean_features.py:96): the host RNG walk and the (synchronous, pageable)
    upload are paid once instead of once per slide -- 60-80 us of a 1.6 ms call."""
    key = (int(n_clusters), int(random_state), str(dev))
    hit = _uniforms_cache.get(key)
    if hit is None:
        u = seeding_draws(n_clusters, n_clusters, random_state)[1]
        if len(_uniforms_cache) >= 64:
            _uniforms_cache.clear()
        hit = _uniforms_cache[key] = (torch.from_numpy(u).to(dev), u.shape[1])      # blocking copy: visible to every stream
    return hit


def _first_center(n_samples, n_clusters, random_state):
    """The first centre of a slide of n_samples patches, the only draw of seeding_draws that depends on the patch count."""
    key = (int(n_samples), int(n_clusters), int(random_state))
    hit = _first_cache.get(key)
    if hit is None:
        if len(_first_cache) >= 8192:
            _first_cache.clear()
        hit = _first_cache[key] = seeding_draws(n_samples, n_clusters, random_state)[0]
    return hit


def _fit(route, X, counts, n_clusters, random_state, max_iter, tol, want_means):
    """One checked call of a C entry on X f32 [rows, D] (rows of the slides back to back): allocates the outputs and the
    workspace.  route "batch": counts = [S, n], S slides of n rows through sq_kmeans_fit; "large": counts = [n], one slide
    through sq_kmeans_fit_large; "ragged": counts = the slides' row counts, through sq_kmeans_fit_ragged.
    Returns labels i32 [rows], cluster_features f32 [S, k, D] (None without want_means), indices i32 [S, k], n_iter i32 [S]."""
    L = _lib.lib()
    D, k, dev = int(X.shape[1]), int(n_clusters), X.device
    if route == "batch":
        S, n = counts
        shape, need = (S, n), L.sq_kmeans_workspace_bytes(S, n, D, k)
    elif route == "large":
        S, n = 1, counts[0]
        shape, need = (n,), L.sq_kmeans_large_workspace_bytes(n, D, k)
        if need == 0:          # a size the entry refuses: let it say why (it names its bound) before anything is allocated
            _lib.check(L.sq_kmeans_fit_large(None, n, D, k, 0, None, 1, max_iter, float(tol), None, None, None, None, None, 0, None))
            raise _lib.SequoiaHipError(f"kmeans (large): unsupported size n={n} dim={D} k={k}")
    else:
        S, n = len(counts), counts[0]
        ns = np.ascontiguousarray(counts, dtype=np.int32)
        firsts = np.array([_first_center(c, k, random_state) for c in counts], dtype=np.int32)
        shape, need = (S, ns), int(L.sq_kmeans_ragged_workspace_bytes(S, ns.ctypes.data, D, k))
    X = X.to(torch.float32).contiguous()
    u_dev, trials = _uniforms(k, random_state, dev)
    first = firsts if route == "ragged" else _first_center(n, k, random_state)
    labels = torch.empty(X.shape[0], dtype=torch.int32, device=dev)
    means = torch.empty(S, k, D, dtype=torch.float32, device=dev) if want_means else None
    seeds = torch.empty(S, k, dtype=torch.int32, device=dev)
    n_iter = torch.empty(S, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    entry = dict(batch=L.sq_kmeans_fit, large=L.sq_kmeans_fit_large, ragged=L.sq_kmeans_fit_ragged)[route]
    _lib.call(entry, dev, X, *shape, D, k, first, u_dev, trials, max_iter, float(tol), labels, means, seeds, n_iter, workspace=ws)
    return dict(labels=labels, cluster_features=means, indices=seeds, n_iter=n_iter)


def kmeans_fit_batch(X, n_clusters=100, random_state=0, max_iter=300, tol=1e-4, want_means=True):
    """X: f32 [S, n, D] CUDA tensor (S slides with the same patch count).  Returns dict of CUDA tensors:
    labels i32 [S, n], cluster_features f32 [S, k, D], indices i32 [S, k], n_iter i32 [S]."""
    _lib.require_gpu()
    if X.dim() == 2:
        X = X.unsqueeze(0)
    if not X.is_cuda:
        raise _lib.SequoiaHipError("kmeans_fit_batch needs a CUDA tensor (no CPU fallback)")
    S, n, D = X.shape
    r = _fit("batch", X.reshape(S * n, D), [S, n], n_clusters, random_state, max_iter, tol, want_means)
    r["labels"] = r["labels"].view(S, n)
    return r


def kmeans_fit(X, n_clusters=100, random_state=0, max_iter=300, tol=1e-4, want_means=True, *, route=None):
    """ONE slide: X f32 [n, D] (or [1, n, D]) CUDA tensor of any patch count up to LARGE_MAX_ROWS.  Returns the dict of
    kmeans_fit_batch for S = 1: labels i32 [1, n], cluster_features f32 [1, k, D], indices i32 [1, k], n_iter i32 [1].

    The kernels are chosen from the row count alone: n <= GRAM_MAX_ROWS runs kmeans_fit_batch (seeding from the slide's
    Gram matrix), larger slides run sq_kmeans_fit_large (per-step candidate distances, chunked member sort; the same
    Lloyd kernels; the size is checked before anything is allocated or copied).  ``route`` is a TEST HOOK, keyword-only:
    "large" sends a small slide through the large-slide entry so that the tests can compare the two routes where both
    exist; "gram" forces the other; leave it None otherwise."""
    _lib.require_gpu()
    if X.dim() == 3 and X.shape[0] == 1:
        X = X[0]
    if X.dim() != 2:
        raise _lib.SequoiaHipError(f"kmeans_fit takes one slide [n, D], got shape {tuple(X.shape)}")
    if not X.is_cuda:
        raise _lib.SequoiaHipError("kmeans_fit needs a CUDA tensor (no CPU fallback)")
    if route not in (None, "gram", "large"):
        raise ValueError(f"route={route!r}")
    large = X.shape[0] > GRAM_MAX_ROWS if route is None else route == "large"
    if not large:
        return kmeans_fit_batch(X.unsqueeze(0), n_clusters, random_state, max_iter, tol, want_means)
    r = _fit("large", X, [int(X.shape[0])], n_clusters, random_state, max_iter, tol, want_means)
    r["labels"] = r["labels"].view(1, -1)
    return r


def _ragged_bytes(counts, D, k):
    arr = np.ascontiguousarray(counts, dtype=np.int32)
    return int(_lib.lib().sq_kmeans_ragged_workspace_bytes(len(arr), arr.ctypes.data, int(D), int(k)))


def ragged_plan(counts, D, n_clusters, max_workspace_bytes):
    """Pure host: cut a list of patch counts, in order, into consecutive groups (lo, hi, route), slides lo..hi-1 per call.
    route "gram": one sq_kmeans_fit_ragged call whose workspace (sq_kmeans_ragged_workspace_bytes) fits
    max_workspace_bytes -- a single slide that alone exceeds the budget is still run, alone; route "large": ONE slide of
    more than GRAM_MAX_ROWS patches, which goes through sq_kmeans_fit_large by itself."""
    counts = [int(c) for c in counts]
    groups = []
    lo = 0
    while lo < len(counts):
        if counts[lo] > GRAM_MAX_ROWS:
            groups.append((lo, lo + 1, "large"))
            lo += 1
            continue
        if _ragged_bytes(counts[lo:lo + 1], D, n_clusters) == 0:
            raise ValueError(f"kmeans (ragged): slide {lo} with n_samples={counts[lo]}, dim={D}, n_clusters={n_clusters} is outside "
                             f"what sq_kmeans_fit_ragged takes (n_clusters <= n_samples, n_clusters <= 256, dim % 4 == 0)")
        hi = lo + 1
        while (hi < len(counts) and hi - lo < RAGGED_MAX_SLIDES and counts[hi] <= GRAM_MAX_ROWS
               and 0 < _ragged_bytes(counts[lo:hi + 1], D, n_clusters) <= max_workspace_bytes):
            hi += 1
        groups.append((lo, hi, "gram"))
        lo = hi
    return groups


def kmeans_fit_ragged(slides, n_clusters=100, random_state=0, max_iter=300, tol=1e-4, want_means=True,
                      max_workspace_bytes=4 << 30):
    """Many slides of DIFFERENT patch counts in one call (the loop over slides of kmean_features.py:65-108).
    slides: a list of f32 [n_i, D] CUDA tensors, or a pair (X_cat [sum n_i, D], counts).  Returns, in the order of the
    input: labels -- a list of i32 [n_i] views of one buffer; cluster_features f32 [S, k, D] (None without want_means);
    indices i32 [S, k]; n_iter i32 [S].  Every slide's results are bit-equal to kmeans_fit of that slide alone.

    ragged_plan cuts the list into consecutive groups whose workspace fits max_workspace_bytes, one
    sq_kmeans_fit_ragged call per group; a slide of more than GRAM_MAX_ROWS patches runs alone through the large-slide
    entry.  The 4 GiB default is a choice, not a measurement: the Gram and distance tables take 12 bytes per pair of
    patches, about 0.2 GB for a 4000-patch slide, so the default holds some twenty of the largest slides
    compute_features_hdf5.py writes, or hundreds of ordinary ones."""
    _lib.require_gpu()
    if isinstance(slides, tuple) and len(slides) == 2 and torch.is_tensor(slides[0]):
        X, counts = slides[0], [int(c) for c in slides[1]]
        if not X.is_cuda:
            raise _lib.SequoiaHipError("kmeans_fit_ragged needs CUDA tensors (no CPU fallback)")
        if X.dim() != 2 or sum(counts) != X.shape[0]:
            raise ValueError(f"kmeans_fit_ragged: X_cat {tuple(X.shape)} does not hold counts summing to {sum(counts)}")
    else:
        slides = list(slides)
        for t in slides:
            if not t.is_cuda:
                raise _lib.SequoiaHipError("kmeans_fit_ragged needs CUDA tensors (no CPU fallback)")
            if t.dim() != 2:
                raise ValueError(f"kmeans_fit_ragged takes slides [n_i, D], got shape {tuple(t.shape)}")
        if len({int(t.shape[1]) for t in slides}) > 1:
            raise ValueError(f"kmeans_fit_ragged: slides of different feature widths {sorted({int(t.shape[1]) for t in slides})}")
        counts = [int(t.shape[0]) for t in slides]
        X = torch.cat([t.to(torch.float32) for t in slides]) if slides else None
    if not counts:
        raise ValueError("kmeans_fit_ragged: empty list of slides")
    for i, n in enumerate(counts):
        if n < n_clusters:
            raise ValueError(f"slide {i}: n_samples={n} should be >= n_clusters={n_clusters}.")
    X = X.to(torch.float32).contiguous()
    S, D, k, dev = len(counts), int(X.shape[1]), int(n_clusters), X.device
    plan = ragged_plan(counts, D, k, max_workspace_bytes)
    rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parts = [_fit("large" if route == "large" else "ragged", X[int(rows[lo]):int(rows[hi])], counts[lo:hi], k, random_state, max_iter, tol,
                  want_means) for lo, hi, route in plan]
    r = parts[0] if len(parts) == 1 else {key: torch.cat([p[key] for p in parts]) if parts[0][key] is not None else None for key in parts[0]}
    r["labels"] = [r["labels"][int(rows[i]):int(rows[i + 1])] for i in range(S)]
    return r


class KMeans:
    """The subset of sklearn.cluster.KMeans the reference touches: constructor (n_clusters,
    random_state), ``fit(X)``, ``labels_``; also ``cluster_features_`` (kmean_features.py:99-105)."""

    def __init__(self, n_clusters=8, random_state=None, max_iter=300, tol=1e-4, device="cuda:0"):
        self.n_clusters = n_clusters
        self.random_state = 0 if random_state is None else random_state
        self.max_iter = max_iter
        self.tol = tol
        self.device = device

    def fit(self, X):
        X = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        if X.shape[0] < self.n_clusters:
            raise ValueError(f"n_samples={X.shape[0]} should be >= n_clusters={self.n_clusters}.")
        r = kmeans_fit(torch.from_numpy(X).to(self.device), self.n_clusters, self.random_state, self.max_iter, self.tol)
        self.labels_ = r["labels"][0].cpu().numpy()
        self.cluster_features_ = r["cluster_features"][0].cpu().numpy()
        self.seed_indices_ = r["indices"][0].cpu().numpy()
        self.n_iter_ = int(r["n_iter"][0])
        return self
