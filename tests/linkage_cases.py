"""Cases of the device average-linkage clustering (sequoia_pub_amd.mapstats.row_distances / linkage_average / cluster_order,
csrc/linkage.hip) and a numpy restatement of what they compute, shared by tests/test_linkage_host.py and
tests/test_gpu_linkage.py.

The restatement is scipy's ``linkage(A, method='average', metric='euclidean')`` followed by ``leaves_list``, rule for rule:
``row_distances`` is pdist's C loop (vectorised over pairs, sequential over features, product and sum rounded separately),
``linkage`` the nearest-neighbour chain with scipy's tie rules, the stable sort of the merges by distance and the
union-find relabelling, ``leaves`` the depth-first walk with the left child first.  tests/golden/linkage.npz holds what
scipy itself gives; tests/golden/make_linkage_golden.py makes it from the inputs defined HERE, which are rebuilt from
their seeds (numpy's RandomState streams are frozen), so the file holds results only."""
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linkage.npz")
GOLDEN_DIST_MAX_K = 130          # scipy's condensed pdist is stored up to this K; above it, its SHA-256


# ---------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------
def row_distances(A):
    """A f64 [K, M] -> f64 [K, K]: sqrt of s, s = s + d * d over the features in ascending order; the diagonal is 0."""
    A = np.asarray(A, dtype=np.float64)
    K, M = A.shape
    s = np.zeros((K, K), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(M):
            d = A[:, t][:, None] - A[:, t][None, :]
            s = s + d * d
        out = np.sqrt(s)
    out[np.arange(K), np.arange(K)] = 0.0
    return out


def condensed(D):
    """The upper triangle of a square [K, K] in pdist's order."""
    K = D.shape[0]
    return D[np.triu_indices(K, 1)]


def first_nonfinite_row(D):
    """The smallest i with a non-finite D[i][j], j > i; -1 if all are finite."""
    bad = np.triu(~np.isfinite(D), 1)
    rows = np.nonzero(bad.any(axis=1))[0]
    return int(rows[0]) if rows.size else -1


def nn_chain(D):
    """D f64 [K, K] symmetric, finite -> (the K-1 merges (a, b, distance, size) in the order they are made, searches)."""
    D = np.array(D, dtype=np.float64)
    K = D.shape[0]
    size = np.ones(K, dtype=np.int64)
    chain, merges, searches = [], [], 0
    idx = np.arange(K)
    for _ in range(K - 1):
        if not chain:
            chain.append(int(np.nonzero(size > 0)[0][0]))
        while True:
            x = chain[-1]
            searches += 1
            live = (size > 0) & (idx != x)
            row = np.where(live, D[x], np.inf)
            dmin = row.min()
            if len(chain) > 1 and not dmin < D[x][chain[-2]]:
                y = chain[-2]                                   # the previous element wins ties
            else:
                y = int(np.nonzero(live & (D[x] == dmin))[0][0])            # the smallest index attaining the minimum
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        a, b = (x, y) if x < y else (y, x)
        na, nb = int(size[a]), int(size[b])
        merges.append((a, b, float(dmin), na + nb))
        size[a], size[b] = 0, na + nb
        upd = (size > 0) & (idx != b)
        new = (float(na) * D[:, a] + float(nb) * D[:, b]) / float(na + nb)  # two products, one sum, one division
        D[upd, b] = new[upd]
        D[b, upd] = new[upd]
    return merges, searches


def relabel(merges, K):
    """The merges sorted by distance (stably) and relabelled with a union-find over 2K-1 labels -> Z f64 [K-1, 4]."""
    order = sorted(range(K - 1), key=lambda r: (merges[r][2], r))
    parent = list(range(2 * K - 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    Z = np.empty((K - 1, 4), dtype=np.float64)
    for row, r in enumerate(order):
        a, b, d, n = merges[r]
        ra, rb = find(a), find(b)
        Z[row] = (min(ra, rb), max(ra, rb), d, n)
        parent[ra] = parent[rb] = K + row
    return Z


def leaves(Z):
    """leaves_list(Z): the depth-first walk from node 2K-2, the left child (Z[., 0]) first -> int32 [K]."""
    K = Z.shape[0] + 1
    out, stack = [], [2 * K - 2]
    while stack:
        node = stack.pop()
        if node < K:
            out.append(node)
        else:
            stack.append(int(Z[node - K, 1]))
            stack.append(int(Z[node - K, 0]))
    return np.array(out, dtype=np.int32)


def linkage(A, return_searches=False):
    """A f64 [K, M] -> (D, Z, leaves) as scipy's pdist, linkage(A, 'average') and leaves_list give them."""
    D = row_distances(A)
    merges, searches = nn_chain(D)
    Z = relabel(merges, D.shape[0])
    out = (D, Z, leaves(Z))
    return out + (searches,) if return_searches else out


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


def correlation_matrix(K, seed):
    """A bit-symmetric correlation matrix [K, K] of correlated noise with a unit diagonal.  The noise is integer, so every
    sum below is exact whatever order a BLAS takes it in, and the rest is one rounded operation per element: the same bits on
    every machine."""
    rs = np.random.RandomState(seed)
    groups = max(1, K // 6)
    n = 3 * K + 7
    x = (rs.randint(-8, 9, (n, K)) + 3 * rs.randint(-4, 5, (n, groups))[:, rs.randint(0, groups, K)]).astype(np.float64)
    m = x.sum(axis=0)
    cov = n * (x.T @ x) - m[:, None] * m[None, :]              # integers below 2^53
    d = np.sqrt(cov.diagonal())
    c = cov / (d[:, None] * d[None, :])
    c[np.arange(K), np.arange(K)] = 1.0
    return c


def block_matrix():
    """48 x 48 of label_i == label_j: nearly every distance is tied."""
    label = np.random.RandomState(301).randint(0, 5, 48)
    return (label[:, None] == label[None, :]).astype(np.float64)


def integer_table():
    """40 x 6 of integers 0..2: many tied distances, some zero."""
    return np.random.RandomState(302).randint(0, 3, (40, 6)).astype(np.float64)


def repeated_rows():
    """33 x 8 with three identical rows and one identical pair: zero distances; the chain empties and restarts."""
    a = np.random.RandomState(303).standard_normal((33, 8))
    a[11] = a[4]
    a[29] = a[4]
    a[20] = a[7]
    return a


def rectangular(K, M, seed):
    return np.random.RandomState(seed).standard_normal((K, M))


SIZES = (2, 3, 5, 17, 63, 64, 65, 130, 257)          # 64: the distance kernel's tile; 63 and 65 its edges
SEARCH_STEP = (1023, 1025)                           # around the search's 1024 threads (K x 8 observations: small inputs)
BOUND = 4096                                         # SQ_MAP_MAX_LINK_ROWS: every LDS array of the linkage at its full extent

CASES = {f"corr_{K}": functools.partial(correlation_matrix, K, 100 + K) for K in SIZES}
CASES.update({f"rect_{K}x8": functools.partial(rectangular, K, 8, 200 + K) for K in SEARCH_STEP})
CASES[f"rect_{BOUND}x4"] = functools.partial(rectangular, BOUND, 4, 200 + BOUND)
CASES.update({"block_48": block_matrix, "integers_40x6": integer_table, "repeated_33x8": repeated_rows,
              "rect_33x8": functools.partial(rectangular, 33, 8, 304)})
TIES = ("block_48", "integers_40x6", "repeated_33x8")


@functools.lru_cache(maxsize=None)
def case(name):
    return _frozen(np.ascontiguousarray(CASES[name](), dtype=np.float64))


@functools.lru_cache(maxsize=None)
def restated(name):
    """(D, Z, leaves, searches) of the restatement, computed once per process and read-only."""
    D, Z, lv, searches = linkage(case(name), return_searches=True)
    return _frozen(D), _frozen(Z), _frozen(lv), searches


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def real_table(n=90, G=66, seed=6):
    """An f32 prediction table [n, G] of eighths, as the mapstats CLI test uses."""
    return (np.random.RandomState(seed).randint(0, 33, (n, G)) * 0.125).astype(np.float32)
