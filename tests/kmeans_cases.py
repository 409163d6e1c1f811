"""Case table and reference of the k-Means sweep: the cluster counts, widths, trial counts and stop rules that km_check
(csrc/kmeans.hip) admits and `cli/kmean_features.py --num_clusters` / `KMeans(n_clusters=8)` hand to the kernels, next to the
one point (k = 100, six trials, dim in {64, 256, 512, 1024, 2048}, max_iter 300, tol 1e-4) the older k-Means tests run at.
Shared by tests/test_kmeans_cases_host.py (CPU: is the reference scikit-learn's, does every row reach its branch, is any
decision marginal, would the table notice the mistakes it is there for), tests/test_gpu_kmeans_sweep.py (GPU: bit equality)
and tests/golden/make_kmeans_sweep.py (the scikit-learn fixture).  No GPU import here.

The reference is oracle/kmeans_oracle.py and nothing else; its optional trace supplies the margins.  Four kinds of case:

    ROWS         whole fits through the public entries, `n_local_trials` following k
    TRIAL_ROWS   whole fits through the C entries with tables of 1 and 8 uniforms per step
    STOP_CASES   max_iter / tol on the slowest-converging row; BATCH_STOP: three slides that stop for different reasons
    DBG_ROWS     Lloyd from given centres (sq_dbg_kmeans_lloyd): the empty-cluster paths no public call reaches

Exact rows: DBG_ROWS built by `_sym` hold small-integer coordinates and every row's negation, so the fp32 column sums are
exactly 0 (`Xc == X`) and every fp64 sum, product and distance below is exact in any order of summation.  A tie on such a
row is a tie in the kernel too, and only there is a tie allowed.  scikit-learn breaks distance ties by `argpartition`'s
internal order, so those rows (DbgRow.sklearn False) have no scikit-learn counterpart by design.

Rows replaced while the table was made are listed at REPLACED with the reason."""
import functools
import math
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import synth  # noqa: E402
from oracle import kmeans_oracle as ko  # noqa: E402

# ----------------------------------------------------------------------------------------------------------------------
# launch constants of csrc/kmeans.hip, each beside the line it mirrors
# ----------------------------------------------------------------------------------------------------------------------
MAX_K = 256                     # `constexpr int KM_MAX_K = 256;`
MAX_TRIALS = 8                  # `constexpr int KM_MAX_TRIALS = 8;`
DOT_SLICES = 8                  # `constexpr int KM_DOT_SLICES = 8;`
DOT_SLICE_MIN_DIM = 32 * DOT_SLICES   # km_lloyd_and_means: `const int ksl = D >= 32 * KM_DOT_SLICES ? KM_DOT_SLICES : 1;`
GEMM_TILE = 64                  # km_dgemm_nt_kernel: `const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;`
GEMM_KC = 32                    # km_dgemm_nt_kernel: `for (int k0 = k_lo; k0 < k_hi; k0 += 32)`
ASSIGN_GROUPS = 16              # km_assign_kernel: `constexpr int G = 16, CB = 7;`
ASSIGN_CB = 7
CENTER_COLS = 64                # `constexpr int KC_ROWS = 128, KC_COLS = 64;`
CENTER_ROWS = 128
NORMS_LANES = 64                # km_center_norms_kernel: `__launch_bounds__(64)`
NORMS_UNROLL = 8                # km_center_norms_kernel: `for (; d + 7 * 64 < D; d += 8 * 64)`
LG_KC = 128                     # `constexpr int KM_LG_KC = 128;`
LG_CHUNK = 1024                 # `constexpr int KM_LG_CHUNK = 1024;`
LG_TILE = 64                    # `constexpr int KM_LG_TILE = 64;`
SEED_LAYOUTS = ((1024, 4, 256), (2048, 2, 1024), (4096, 4, 1024))     # `KM_SEED_LAYOUTS[]`: max_rows, pts, threads
GRAM_MAX_N = 4096               # `constexpr int KM_GRAM_MAX_N = 4096;`
LARGE_MAX_N = 65536             # `#define SQ_KMEANS_LARGE_MAX_SAMPLES 65536`
FIRST_BURST, BURST = 2, 4       # km_lloyd_and_means: `const int burst = it == 0 ? 2 : 4;`
SUMS_UNROLL = 8                 # km_sums_kernel: `for (; i + 8 <= hi; i += 8)`

GUARD = 64                      # sentinel elements on both sides of every output
SENT_I32 = -0x5A5A5A5B          # guard pattern of the int32 outputs
SENT_F32_BITS = 0x7FA5C3E1      # guard pattern of the float32 outputs (a NaN with a payload no kernel produces)


def trials_of(k):
    """kmeans.py seeding_draws: `trials = 2 + int(np.log(n_clusters))` (_kmeans.py:225)."""
    return 2 + int(math.log(k))


def seed_class(n):
    """km_seed_class: the first layout whose max_rows holds n; 1-based as the issue counts them."""
    for c, (rows, _, _) in enumerate(SEED_LAYOUTS):
        if n <= rows:
            return c + 1
    return None                  # the large route only


def facts(n, dim, k):
    """What the launches of one fit of (n, dim, k) look like, from the constants above alone."""
    ksl = DOT_SLICES if dim >= DOT_SLICE_MIN_DIM else 1
    # km_dgemm_nt_kernel: `const int kper = ((K + ksl - 1) / ksl + 31) / 32 * 32;`
    kper = ((dim + ksl - 1) // ksl + GEMM_KC - 1) // GEMM_KC * GEMM_KC
    slices = [(s * kper, min(dim, s * kper + kper)) for s in range(ksl)]
    groups = [((g + 1) * k // ASSIGN_GROUPS) - (g * k // ASSIGN_GROUPS) for g in range(ASSIGN_GROUPS)]
    cls = seed_class(n)
    return dict(
        ksl=ksl, kper=kper,
        empty_slices=sum(1 for lo, hi in slices if lo >= hi),
        gemm_k_tail=any(lo < hi and (hi - lo) % GEMM_KC for lo, hi in slices),          # a K step with `kk < k_hi` false for some loads
        m_tiles=(k + GEMM_TILE - 1) // GEMM_TILE, m_last_rows=(k - 1) % GEMM_TILE + 1,
        n_tiles=(n + GEMM_TILE - 1) // GEMM_TILE, n_last_cols=(n - 1) % GEMM_TILE + 1,
        assign_empty_groups=sum(1 for g in groups if g == 0), assign_max_group=max(groups),
        assign_partial_batch=any(g % ASSIGN_CB for g in groups if g),                   # `c0 + u < c_hi ? c0 + u : c_hi - 1`
        center_blocks=(dim + CENTER_COLS - 1) // CENTER_COLS, center_last_cols=(dim - 1) % CENTER_COLS + 1,
        center_row_tiles=(n + CENTER_ROWS - 1) // CENTER_ROWS,
        norms_unrolled_rounds=max(0, (dim - (NORMS_UNROLL - 1) * NORMS_LANES + NORMS_UNROLL * NORMS_LANES - 1)
                                  // (NORMS_UNROLL * NORMS_LANES)),                      # rounds of lane 0
        norms_tail_lanes=_norms_tail_lanes(dim),
        lg_k_tail=dim % LG_KC, lg_k_chunks=(dim + LG_KC - 1) // LG_KC,
        lg_chunks=(n + LG_CHUNK - 1) // LG_CHUNK, lg_tiles=(n + LG_TILE - 1) // LG_TILE,
        lg_last_chunk_points=(n - 1) % LG_CHUNK + 1, lg_last_tile_points=(n - 1) % LG_TILE + 1,
        seed_class=cls, seed_vec4=bool(cls and SEED_LAYOUTS[cls - 1][1] == 4 and n % 4 == 0),
        seed_steps=k - 1, trials=trials_of(k))


def _norms_tail_lanes(dim):
    """Lanes of km_center_norms_kernel that run the scalar loop behind the unrolled one at least once."""
    lanes = 0
    for lane in range(NORMS_LANES):
        d = lane
        while d + (NORMS_UNROLL - 1) * NORMS_LANES < dim:
            d += NORMS_UNROLL * NORMS_LANES
        lanes += d < dim
    return lanes


# ----------------------------------------------------------------------------------------------------------------------
# ROWS: whole fits, data from synth.features_<kind>(seed, n, dim)
# ----------------------------------------------------------------------------------------------------------------------
Row = namedtuple("Row", "name kind seed n dim k branch expect")
ROWS = [
    Row("k1", "gmm", 301, 64, 516, 1, "k = 1: no seeding step, one centre, the centre-norm loop's unrolled round plus a 4-lane tail",
        dict(seed_steps=0, assign_empty_groups=15, norms_unrolled_rounds=1, norms_tail_lanes=4, empty_slices=2)),
    Row("k2", "lowrank", 302, 500, 132, 2, "k = 2: fourteen empty centre groups, two trials",
        dict(trials=2, assign_empty_groups=14, gemm_k_tail=True, ksl=1)),
    Row("k3_n2049", "gmm", 303, 2049, 8, 3, "seeding class 3 with n % 4 != 0 (scalar loads), three trials",
        dict(seed_class=3, seed_vec4=False, trials=3)),
    Row("k8_dim36", "normal", 304, 257, 36, 8, "k < 16: eight empty centre groups; dim % 32 tail of the product",
        dict(assign_empty_groups=8, gemm_k_tail=True, n_last_cols=1)),
    Row("k15_dim252", "lowrank", 305, 1000, 252, 15, "ksl = 1 just below the slicing threshold of 256, seven full K steps and a 28 tail",
        dict(ksl=1, gemm_k_tail=True, assign_empty_groups=1)),
    Row("k17_dim68", "lowrank", 306, 1025, 68, 17, "seeding class 2 lower edge; second centring block with 4 live columns",
        dict(seed_class=2, center_blocks=2, center_last_cols=4, assign_empty_groups=0)),
    Row("k129_dim260", "lowrank", 360, 400, 260, 129, "third 64-row M tile with one live row; slices 5..7 empty at dim 260",
        dict(m_tiles=3, m_last_rows=1, ksl=8, empty_slices=3, gemm_k_tail=True)),
    Row("k256_dim4", "normal", 308, 300, 4, 256, "smallest dim with the largest k: seven trials, 16 centres per group",
        dict(trials=7, assign_max_group=16, m_tiles=4, lg_k_tail=4)),
    Row("n_eq_k256", "normal", 309, 256, 4, 256, "n = k at the maximum: every point a centre",
        dict(trials=7, seed_steps=255)),
    Row("class1_top", "gmm", 310, 1024, 12, 100, "seeding class 1 upper edge",
        dict(seed_class=1, seed_vec4=True)),
    Row("class2_top", "lowrank", 311, 2048, 12, 16, "seeding class 2 upper edge",
        dict(seed_class=2, assign_empty_groups=0)),
    Row("k255_n4093", "normal", 312, 4093, 8, 255, "seeding class 3 with scalar loads, seven trials, centre groups of 15 and 16",
        dict(seed_class=3, seed_vec4=False, trials=7, m_last_rows=63)),
    Row("dim1028", "gmm", 313, 200, 1028, 5, "slice 7 empty and a 4-wide K tail at dim 1028; two unrolled norm rounds plus a tail",
        dict(ksl=8, empty_slices=1, gemm_k_tail=True, norms_unrolled_rounds=2, norms_tail_lanes=4, lg_k_tail=4)),
    Row("large_4097", "gmm", 314, 4097, 4, 3, "large route only: five chunks and 65 tiles, the last of each holding one point",
        dict(seed_class=None, lg_chunks=5, lg_tiles=65, lg_last_chunk_points=1, lg_last_tile_points=1)),
    # company for the ragged calls: with class2_top one call of (dim 12, k 16) spans all three seeding classes
    Row("class1_k16", "lowrank", 315, 600, 12, 16, "seeding class 1 next to class2_top in one ragged call",
        dict(seed_class=1)),
    Row("class3_k16", "lowrank", 316, 2049, 12, 16, "seeding class 3 next to class2_top in one ragged call",
        dict(seed_class=3, seed_vec4=False)),
]
ROW = {r.name: r for r in ROWS}
REPLACED = [                    # (name, old data, new data, why)
    ("k129_dim260", "gmm 307", "lowrank 360",
     "round_gap 8.6e-16 at seeding step 102: the fp64 sum behind one candidate's potential, 25381.846679687522, lies 2e-11 above an "
     "fp32 rounding boundary.  The 2e-11 is the oracle's own distance of a chosen centre to itself (norms by einsum, dot products "
     "by matmul: they do not cancel to the last bit; the kernels take both from one product and get exactly 0), so the oracle "
     "rounds up where an exact sum would round to even.  Late steps of a small slide with many centres sum a few hundred fp32 "
     "values of one magnitude, which lands on such a boundary about once in 2^10 potentials: gmm 347-350 and 360-367 failed "
     "the same floor, lowrank 360 is the first data that passes every floor and agrees with scikit-learn."),
]


def ragged_groups():
    """Rows that share (dim, k) and fit the Gram route, in table order: one sq_kmeans_fit_ragged call each."""
    by = {}
    for r in ROWS:
        if r.n <= GRAM_MAX_N:
            by.setdefault((r.dim, r.k), []).append(r)
    return [g for g in by.values() if len(g) > 1]


# TRIAL_ROWS: n_local_trials away from 2 + int(log k); uniforms = RandomState(0).uniform(size=(k - 1, T)), first centre FIRST
TrialRow = namedtuple("TrialRow", "name kind seed n dim k trials first branch")
TRIAL_ROWS = [
    TrialRow("trials1", "gmm", 320, 600, 20, 12, 1, 17, "one trial per step: the argmin over candidates has nothing to choose"),
    TrialRow("trials8", "gmm", 321, 600, 20, 12, 8, 17, "eight trials per step: every slot of the KM_MAX_TRIALS arrays is live"),
]

# STOP_CASES on the slowest-converging row (52 iterations with the defaults): (name, max_iter, tol, why)
STOP_ROW = "k17_dim68"
StopCase = namedtuple("StopCase", "name max_iter tol branch")
STOP_TOL = 1.0                  # stops by shift <= tol well before the labels settle (the host test asserts iteration >= 2)
STOP_CASES = [
    StopCase("max_iter0", 0, 1e-4, "no iteration: n_iter = 0, labels from the seeds"),
    StopCase("max_iter1", 1, 1e-4, "stops inside the first burst of 2"),
    StopCase("max_iter2", 2, 1e-4, "stops at the end of the first burst"),
    StopCase("max_iter3", 3, 1e-4, "one past the first burst: inside the first burst of 4"),
    StopCase("max_iter6", 6, 1e-4, "the end of the second burst (2 + 4)"),
    StopCase("max_iter7", 7, 1e-4, "one past the second burst"),
    StopCase("tol0", 300, 0.0, "tol = 0: only the label rule stops the loop"),
    StopCase("tol_shift", 300, STOP_TOL, "stops by shift <= tol, not by labels"),
]

# BATCH_STOP: one sq_kmeans_fit call of three equal-n slides whose stop reasons differ under max_iter
BatchStop = namedtuple("BatchStop", "kinds seeds n dim k max_iter")
BATCH_STOP = BatchStop(("gmm", "lowrank", "gmm"), (330, 331, 332), 300, 36, 8, 12)


@functools.lru_cache(maxsize=None)
def data(kind, seed, n, dim):
    X = getattr(synth, "features_" + kind)(seed, n, dim)
    X.setflags(write=False)
    return X


def row_data(r):
    return data(r.kind, r.seed, r.n, r.dim)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def fit_reference(kind, seed, n, dim, k, max_iter=300, tol=1e-4):
    """ko.kmeans_fit of one slide with its trace: labels, indices, n_iter, centers_c (centred), cluster_means, trace.  Computed
    once per process and handed out read-only."""
    X = data(kind, seed, n, dim)
    trace = {}
    o = ko.kmeans_fit(X, k, 0, max_iter, tol, trace=trace)
    Xc, mean = ko.center_data(X)
    centers_c = ko.lloyd(Xc, Xc[o["indices"]], trace["tol"], max_iter)[1]
    return _freeze(dict(labels=o["labels"].astype(np.int32), indices=o["indices"].astype(np.int32), n_iter=int(o["n_iter"]),
                        centers_c=centers_c, cluster_means=ko.cluster_means(X, o["labels"], k), trace=trace))


def row_reference(r, max_iter=300, tol=1e-4):
    return fit_reference(r.kind, r.seed, r.n, r.dim, r.k, max_iter, tol)


def trial_table(k, trials):
    return np.random.RandomState(0).uniform(size=(k - 1, trials))


@functools.lru_cache(maxsize=None)
def trial_reference(name):
    """ko.kmeans_plusplus with the row's own table, then ko.lloyd from those seeds."""
    r = {t.name: t for t in TRIAL_ROWS}[name]
    X = data(r.kind, r.seed, r.n, r.dim)
    Xc, _ = ko.center_data(X)
    trace = {}
    idx = ko.kmeans_plusplus(Xc, r.k, r.first, trial_table(r.k, r.trials), trace)
    tol_ = ko.tolerance(X, 1e-4)
    labels, centers, n_iter = ko.lloyd(Xc, Xc[idx], tol_, 300, trace)
    trace["tol"] = tol_
    return _freeze(dict(labels=labels.astype(np.int32), indices=idx.astype(np.int32), n_iter=int(n_iter), centers_c=centers,
                        cluster_means=ko.cluster_means(X, labels, r.k), trace=trace))


# ----------------------------------------------------------------------------------------------------------------------
# DBG_ROWS: Lloyd from given centres.  X [S, n, dim] raw, C [S, k, dim] centred.
# ----------------------------------------------------------------------------------------------------------------------
DbgRow = namedtuple("DbgRow", "name build max_iter tol sklearn branch")


def _sym(points):
    """Small-integer rows and their negations, interleaved (p0, -p0, p1, -p1, ...): the fp32 column mean is exactly 0."""
    P = np.asarray(points, dtype=np.float32)
    X = np.empty((2 * len(P), P.shape[1]), np.float32)
    X[0::2], X[1::2] = P, -P
    return X


def _pushed(kind, seed, n, dim, k, far, pick_seed=0):
    """Centres = k data rows (centred), the rows listed in `far` moved 1000 away along all axes: they start empty."""
    X = data(kind, seed, n, dim)
    Xc, _ = ko.center_data(X)
    idx = np.random.RandomState(pick_seed).choice(n, k, replace=False)
    C = Xc[idx].copy()
    for j, c in enumerate(far):
        C[c] += np.float32(1000.0 + 100.0 * j)
    return X[None], C[None]


def _one_empty():
    return _pushed("gmm", 340, 200, 36, 6, [2])


def _three_empty_shared_donor():
    return _pushed("gmm", 341, 240, 20, 7, [1, 4, 5], pick_seed=3)


def _k1():
    X = data("normal", 342, 70, 12)
    return X[None], np.full((1, 1, 12), 3.0, np.float32)


def _tie_farthest():
    # one live centre at the origin, four points at the same distance 5 (and their negations: eight), two empty clusters:
    # the two lowest indices among the eight must move.  Rows 0..7 are the ties, the rest lies closer.
    pts = [[3, 4, 0, 0], [0, 0, 5, 0], [4, 0, 0, 3], [0, 5, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0], [2, 0, 0, 1]]
    X = _sym(pts)
    C = np.zeros((3, 4), np.float32)
    C[1], C[2] = [100, 0, 0, 0], [0, 100, 0, 0]
    return X[None], C[None]


def _all_zero_heaviest():
    # every point sits on its centre (distances all 0): relocation is skipped, the two empty clusters copy the new row of
    # the heaviest cluster.  A row and its negation come equally often, so only the origin can be heaviest alone: cluster 4,
    # six members, against three and four.
    base = np.concatenate([_sym([[2, 1, 0, 0], [0, 3, 1, 0]]), np.zeros((1, 4), np.float32)])      # p0, -p0, p1, -p1, 0
    reps = [3, 3, 4, 4, 6]
    X = np.concatenate([np.repeat(base[i:i + 1], reps[i], axis=0) for i in range(5)])
    C = np.concatenate([base, [[50, 50, 0, 0], [0, 0, 60, 0]]]).astype(np.float32)
    return X[None], C[None]


def _two_heaviest_equal():
    # as above without the origin: clusters 2 and 3 (p1 and -p1, five members each) are both heaviest, np.argmax takes 2
    base = _sym([[2, 1, 0, 0], [0, 3, 1, 0]])
    reps = [3, 3, 5, 5]
    X = np.concatenate([np.repeat(base[i:i + 1], reps[i], axis=0) for i in range(4)])
    C = np.concatenate([base, [[50, 50, 0, 0]]]).astype(np.float32)
    return X[None], C[None]


def _duplicate_centres():
    # centres 1 and 3 are the same row: every point they are nearest to takes label 1, cluster 3 starts empty and is refilled
    X = _sym([[6, 0, 0, 1], [5, 1, 0, 0], [0, 7, 1, 0], [0, 6, 0, 2], [1, 0, 9, 0], [0, 1, 8, 0], [12, 0, 0, 0]])
    C = np.array([[-5, 0, 0, 0], [5, 0, 0, 0], [0, 6, 0, 0], [5, 0, 0, 0], [0, -6, 0, 0]], np.float32)
    return X[None], C[None]


def _short_of_far_points():
    # three empty clusters and TWO points off their centres: the first two relocations take them, the third takes a point at
    # distance 0, the lowest index (np.max(distances) == 0 is asked once, before the loop)
    # Row 0, the point that moves at distance 0, lies in a LIGHT cluster (0: two copies and the far point; the heaviest is
    # cluster 2 with four): a relocation that stops at distance 0 leaves cluster 6 with the heaviest cluster's row instead
    # of row 0, the next update's shift is 0 and the loop ends one iteration early.
    base = _sym([[2, 1, 0, 0], [0, 3, 1, 0]])
    reps = [2, 2, 4, 4]
    X = np.concatenate([np.repeat(base[i:i + 1], reps[i], axis=0) for i in range(4)])
    X = np.concatenate([X, _sym([[3, 1, 0, 0]])])             # [3,1,0,0] joins cluster 0 at distance 1, its negation cluster 1
    C = np.concatenate([base, [[50, 50, 0, 0], [0, 0, 60, 0], [0, 70, 0, 0]]]).astype(np.float32)
    return X[None], C[None]


def _strict_while_relocating():
    # Cluster 1 holds three copies of q = (10,0,0,0) under a centre 8 away; cluster 3 is empty.  Iteration 1 moves the first
    # copy to cluster 3, so centres 1 and 3 both become q; iteration 2 gives every copy back to cluster 1 (lower index):
    # the labels repeat, the stop is strict -- and the same iteration's update relocates (0,7,0,0) from cluster 0 to the
    # again empty cluster 3.  The labels of a strict stop are kept; an E-step against the final centres would move that point.
    q = [10, 0, 0, 0]
    X = _sym([q, q, q, [0, 5, 0, 0], [0, 7, 0, 0]])
    C = np.array([[0, 0, 0, 0], [10, 0, 8, 0], [-10, 0, 0, 0], [0, 0, 0, 100]], np.float32)
    return X[None], C[None]


def _line(scale):
    """A line of points (coordinate 0) on which cluster A = {4, 20} holds both points in iteration 1 and loses both in
    iteration 2 (4 goes back to B at 0, 20 to C which has moved from 40 to 26), mirrored through the origin: clusters 1 and 3
    are empty in iteration 2 and the two farthest points are mirror images at equal distance."""
    pts = [[4, 0, 0, 0], [20, 0, 0, 0], [26, 1, 0, 0], [26, 0, 1, 0], [1, 0, 0, 1], [0, 1, 0, 0]]
    X = _sym(pts) * np.float32(scale)
    C = np.array([[0, 0, 0, 0], [5, 0, 0, 0], [40, 0, 0, 0], [-5, 0, 0, 0], [-40, 0, 0, 0]], np.float32) * np.float32(scale)
    return X, C


def _batch_converged_and_relocating():
    # slide 0 starts from the centres slide 1 ends at: its first update moves nothing, shift = 0 <= tol, done after iteration
    # 1; slides 1 and 2 (the same line, once doubled) relocate two clusters in iteration 2
    X1, C1 = _line(1)
    X2, C2 = _line(2)
    C0 = ko.lloyd(X1, C1, 0.0, 300)[1]
    return np.stack([X1, X1, X2]), np.stack([C0, C1, C2])


DBG_ROWS = [
    DbgRow("one_empty", _one_empty, 300, 1e-4, True, "one empty cluster takes the farthest point"),
    DbgRow("three_empty", _three_empty_shared_donor, 300, 1e-4, True,
           "three empty clusters in one iteration, two of the farthest points leave the same donor cluster"),
    DbgRow("k1", _k1, 300, 1e-4, True, "k = 1 from a centre that is no data row"),
    DbgRow("tie_farthest", _tie_farthest, 300, 1e-4, False, "equal farthest distances: the lower index moves"),
    DbgRow("all_zero", _all_zero_heaviest, 300, 1e-4, False,
           "all distances zero: relocation skipped, empty clusters copy the heaviest cluster's new row"),
    DbgRow("two_heaviest", _two_heaviest_equal, 300, 1e-4, False, "two heaviest clusters of equal weight: the first maximum wins"),
    DbgRow("dup_centres", _duplicate_centres, 300, 1e-4, False, "duplicate initial centres: the lower index wins every point"),
    DbgRow("short_of_far", _short_of_far_points, 300, 1e-4, False,
           "fewer points off their centre than empty clusters: the rest move at distance 0, lowest index first"),
    DbgRow("strict_relocating", _strict_while_relocating, 300, 1e-4, False,
           "a strict stop in an iteration that relocates: the kept labels differ from an E-step against the final centres"),
    DbgRow("batch_mixed", _batch_converged_and_relocating, 300, 0.0, False,
           "S = 3: slide 0 is done after iteration 1 while slides 1 and 2 relocate in iteration 2"),
]
DBG = {r.name: r for r in DBG_ROWS}


@functools.lru_cache(maxsize=None)
def dbg_inputs(name):
    X, C = DBG[name].build()
    X = np.ascontiguousarray(X, np.float32)
    C = np.ascontiguousarray(C, np.float32)
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


@functools.lru_cache(maxsize=None)
def dbg_reference(name, lloyd=None):
    """Per slide ko.lloyd(ko.center_data(X)[0], C, tol(X)): labels [S, n], centers [S, k, dim], n_iter [S], cluster_means, traces.
    lloyd: another Lloyd of the same signature (the mutants of the host test)."""
    r = DBG[name]
    X, C = dbg_inputs(name)
    out = dict(labels=[], centers=[], n_iter=[], cluster_means=[], traces=[])
    for s in range(X.shape[0]):
        Xc, _ = ko.center_data(X[s])
        trace = {}
        tol_ = ko.tolerance(X[s], r.tol)
        labels, centers, n_iter = (lloyd or ko.lloyd)(Xc, C[s], tol_, r.max_iter, trace)
        trace["tol"] = tol_
        out["labels"].append(labels.astype(np.int32))
        out["centers"].append(centers)
        out["n_iter"].append(int(n_iter))
        out["cluster_means"].append(ko.cluster_means(X[s], labels, C.shape[1]))
        out["traces"].append(trace)
    return _freeze(dict(labels=np.stack(out["labels"]), centers=np.stack(out["centers"]), n_iter=np.array(out["n_iter"], np.int32),
                        cluster_means=np.stack(out["cluster_means"]), traces=out["traces"]))


# ----------------------------------------------------------------------------------------------------------------------
# margins: how far every decision of a traced fit lies from flipping
# ----------------------------------------------------------------------------------------------------------------------
# The kernels and the oracle take the same fp64 sums in different orders.  Reassociating a sum of m terms moves it by at
# most about m * 2^-53 of the sum of the terms' magnitudes (Higham, Accuracy and Stability, (4.4)); a decision is safe when
# its gap is SAFETY times that.  SAFETY = 8 on top of a worst-case bound (all terms are non-negative here, so the bound is
# m * 2^-53 RELATIVE; observed reassociation errors are a few ulps): a larger factor would reject rows by chance alone, since
# among the ~1800 potentials of a k = 255 row the one nearest to an fp32 rounding boundary lies about 2^-24 / 1800 = 3e-11
# from it, relative, against m * 2^-53 = 4.5e-13 at m = 4093.
# The potentials are fl32 of such a sum.  The fp32 value is the same in any order of summation when the fp64 sum stays clear
# of the fp32 rounding boundaries (`round_gap`); then every comparison of potentials sees the same bits, and equal fp32
# potentials of distinct candidates are a tie the first-minimum rule decides the same way everywhere.  The gap between the
# best and the runner-up among distinct candidates is taken on the fp64 sums.
SAFETY = 8.0
EPS64 = 2.0 ** -53


def floor_sum(m):
    """Relative floor for a decision that hangs on an fp64 sum of m non-negative terms."""
    return SAFETY * m * EPS64


def _round_gap(s):
    """Relative distance of the fp64 values s from the nearest boundary of fp32 round-to-nearest."""
    s = np.atleast_1d(np.asarray(s, np.float64))
    f = s.astype(np.float32)
    up = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    dn = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
    return np.minimum(up - s, s - dn) / np.maximum(np.abs(s), 1e-300)


def seeding_margins(trace, n):
    """(smallest relative gap between the best and the runner-up potential among DISTINCT candidates, on the fp64 sums;
        smallest relative distance of a potential's fp64 sum from an fp32 rounding boundary, over the sums that are not
        exact in any order (the trace's `potential_exact`);
        smallest gap between u * pot and the neighbouring cumulative sums, relative to pot)."""
    pot_gap, round_gap, cum_gap = np.inf, np.inf, np.inf
    if "first_potential_sum" in trace and not trace["first_potential_exact"]:
        round_gap = float(_round_gap(trace["first_potential_sum"]).min())
    for s in trace.get("seeding", []):
        cand, sums = s["candidates"], s["potential_sums"]
        best = s["chosen"]
        other = sums[cand != cand[best]]
        if len(other):
            pot_gap = min(pot_gap, float(abs(other.min() - sums[best]) / max(sums[best], 1e-300)))
        live = ~s["potential_exact"]                            # an exact sum is the same in any order: it rounds one way
        if live.any():
            round_gap = min(round_gap, float(_round_gap(sums[live]).min()))
        rv, lo, hi = s["rand_vals"], s["cum_below"], s["cum_at"]
        gaps = np.concatenate([(rv - lo)[cand > 0], np.abs(hi - rv)])      # a clipped candidate: u * pot lies beyond the last sum
        cum_gap = min(cum_gap, float(gaps.min() / s["pot"]))
    return pot_gap, round_gap, cum_gap


def lloyd_margins(trace, Xc, exact=False):
    """(smallest (runner_up - best) / (|x|^2 + max |c|^2) over all points and E-steps -- the reassociation error of
    |c|^2 - 2 x.c over dim terms is at most dim * 2^-53 * (|x|^2 + 2 |c|^2), by Cauchy-Schwarz;
    smallest |shift - tol| / tol over the iterations; the same over max(shift, tol), the scale of the sum that is compared).
    exact: designed ties allowed -- gaps of exactly 0 are skipped (exact rows only)."""
    x2 = np.einsum("ij,ij->i", Xc.astype(np.float64), Xc.astype(np.float64))
    gap_min, shift_min, shift_strict = np.inf, np.inf, np.inf
    tol = trace["tol"]
    for rec in trace.get("lloyd", []):
        gap = rec["runner_up"] - rec["best"]
        scale = x2 + 2.0 * float(np.abs(rec["center_norms"]).max()) + 1e-300
        rel = gap / scale
        if exact:
            rel = rel[gap != 0]
        if len(rel):
            gap_min = min(gap_min, float(rel.min()))
        if not rec["final"] and tol > 0:
            shift_min = min(shift_min, abs(rec["shift"] - tol) / tol)
            shift_strict = min(shift_strict, abs(rec["shift"] - tol) / max(rec["shift"], tol))
    return gap_min, shift_min, shift_strict


def traced_cases():
    """Every traced fit of the table: (tag, n, dim, k, trace, Xc, exact)."""
    for r in ROWS:
        yield "row/" + r.name, r.n, r.dim, r.k, row_reference(r)["trace"], ko.center_data(row_data(r))[0], False
    stop = ROW[STOP_ROW]
    for c in STOP_CASES:
        yield ("stop/" + c.name, stop.n, stop.dim, stop.k, row_reference(stop, c.max_iter, c.tol)["trace"],
               ko.center_data(row_data(stop))[0], False)
    b = BATCH_STOP
    for s, (kind, seed) in enumerate(zip(b.kinds, b.seeds)):
        yield (f"batch/{s}", b.n, b.dim, b.k, fit_reference(kind, seed, b.n, b.dim, b.k, b.max_iter)["trace"],
               ko.center_data(data(kind, seed, b.n, b.dim))[0], False)
    for t in TRIAL_ROWS:
        yield "trial/" + t.name, t.n, t.dim, t.k, trial_reference(t.name)["trace"], ko.center_data(data(t.kind, t.seed, t.n, t.dim))[0], False
    for d in DBG_ROWS:
        X, C = dbg_inputs(d.name)
        for s, trace in enumerate(dbg_reference(d.name)["traces"]):
            yield f"dbg/{d.name}/{s}", X.shape[1], X.shape[2], C.shape[1], trace, ko.center_data(X[s])[0], not d.sklearn


def margin_floors(n, dim, k):
    """The admitted floor of each margin of margin_record, from the length of the fp64 sum the decision hangs on."""
    return dict(pot_gap=floor_sum(n), round_gap=floor_sum(n), cum_gap=floor_sum(n), dist_gap=floor_sum(dim), shift=floor_sum(k * dim))


def margin_record(n, trace, Xc, exact):
    pot_gap, round_gap, cum_gap = seeding_margins(trace, n)
    dist_gap, shift_tol, shift = lloyd_margins(trace, Xc, exact)
    return dict(pot_gap=pot_gap, round_gap=round_gap, cum_gap=cum_gap, dist_gap=dist_gap, shift=shift, shift_over_tol=shift_tol)


def stop_lloyd(case, lloyd):
    """The Lloyd part of one STOP_CASES fit through `lloyd` (ko.lloyd or a mutant): the seeds do not depend on the stop rule."""
    r = ROW[STOP_ROW]
    X = row_data(r)
    Xc, _ = ko.center_data(X)
    return lloyd(Xc, Xc[row_reference(r)["indices"]], ko.tolerance(X, case.tol), case.max_iter)


# ----------------------------------------------------------------------------------------------------------------------
# mutants of ko.lloyd: the mistakes the table is there to see
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("last_minimum", "last_maximum", "ascending_relocation", "ties_by_higher_index", "no_final_e_step", "strict_not_restored",
           "relocation_stops_at_zero")


def lloyd_mutant(mutant):
    """ko.lloyd with one rule changed (None: unchanged, to show the copy is faithful)."""
    assert mutant is None or mutant in MUTANTS

    def assign(X64, centers32):
        C64 = centers32.astype(np.float64)
        cn = np.einsum("ij,ij->i", C64, C64)
        pd = cn[None, :] - 2.0 * (X64 @ C64.T)
        if mutant == "last_minimum":
            return (pd.shape[1] - 1 - np.argmin(pd[:, ::-1], axis=1)).astype(np.int32)
        return np.argmin(pd, axis=1).astype(np.int32)

    def run(Xc, centers_init, tol, max_iter=300, trace=None):
        n, k = Xc.shape[0], centers_init.shape[0]
        X64 = Xc.astype(np.float64)
        centers = centers_init.astype(np.float32).copy()
        labels_old = np.full(n, -1, dtype=np.int32)
        labels = labels_old
        strict = False
        n_iter = 0
        for it in range(max_iter):
            n_iter = it + 1
            labels = assign(X64, centers)
            sums = np.zeros((k, Xc.shape[1]), dtype=np.float64)
            np.add.at(sums, labels, X64)
            weight = np.bincount(labels, minlength=k).astype(np.float64)
            empty = np.where(weight == 0)[0]
            if len(empty) > 0:
                dist = ((Xc - centers[labels]) ** 2).sum(axis=1, dtype=np.float64)
                if dist.max() > 0:
                    order = np.arange(n)
                    if mutant == "ties_by_higher_index":
                        order = -order
                    key = dist if mutant == "ascending_relocation" else -dist
                    far = np.lexsort((order, key))[:len(empty)]
                    if mutant == "relocation_stops_at_zero":
                        far = far[dist[far] > 0]
                    for new_id, far_idx in zip(empty, far):
                        old_id = labels[far_idx]
                        sums[old_id] -= X64[far_idx]
                        sums[new_id] = X64[far_idx]
                        weight[new_id] = 1
                        weight[old_id] -= 1
            new = np.empty_like(centers)
            amax = int(np.argmax(weight))
            if mutant == "last_maximum":
                amax = int(k - 1 - np.argmax(weight[::-1]))
            for j in range(k):
                if weight[j] > 0:
                    new[j] = (sums[j] / weight[j]).astype(np.float32)
            for j in range(k):
                if not weight[j] > 0:
                    new[j] = new[amax]
            shift_tot = float(((new.astype(np.float64) - centers.astype(np.float64)) ** 2).sum())
            centers = new
            if np.array_equal(labels, labels_old):
                strict = True
                break
            if shift_tot <= tol:
                break
            labels_old = labels
        if mutant == "strict_not_restored":
            labels = assign(X64, centers)          # the forced closing E-step kept for a strictly converged slide as well
        elif not strict and mutant != "no_final_e_step":
            labels = assign(X64, centers)
        if max_iter <= 0 and mutant == "no_final_e_step":
            labels = assign(X64, centers)          # nothing ran at all: keep the labels defined
        return labels, centers, n_iter
    return run
