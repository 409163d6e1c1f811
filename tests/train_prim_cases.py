"""Case tables and float64 references of the five training-step entries -- sq_mse_loss_grad, sq_adamw_step, sq_batch_metrics
(csrc/train.hip), sq_cast_f32_to_bf16, sq_cast_bf16_to_f32 (csrc/elementwise.hip) -- shared by tests/test_train_prim_host.py
(CPU: are the references right, do the inputs meet their conditions, what does torch's own fp32 AdamW lose against float64?) and
tests/test_gpu_train_prims.py (GPU: each entry alone, through the C ABI).  No GPU import here.

References are plain NumPy in float64.  Where the operation itself contains a float32 rounding (the MSE difference and
gradient) the reference performs that rounding; the casts are torch's CPU conversions, compared as bit patterns.

Beyond the listed MSE sizes one case (`stagnation`) gives every thread eight or nine terms, a 1 and then squares just under 2^-24:
at the listed sizes a thread sums at most three terms, and a float32 accumulator would stay inside the 2^-22 loss bound.

AdamW hyperparameters are the float32 values the C entry receives, widened to double (`f32`): the kernel forms 1 - beta and
beta^step from those floats.  torch forms them from the Python doubles, so against torch run with beta2 = 0.999 (the double)
the second moment sits about 1.3e-5 relative lower; `adamw_torch(..., double_hyper=True)` measures that.

Units of the AdamW bounds, per element, t = steps taken:
    p:  t * (ulp32(running max of |p| over the states before and after every step) + lr * 2^-24)
    m:  t * 2^-24 * running max of |g * grad_scale|
    v:  t * 2^-24 * v_ref
TORCH_UNITS records the worst deviation of torch.optim.AdamW(foreach=False) on CPU float32 from the float64 reference in these
units over all cases below (test_train_prim_host.py measures it again and holds the record to it); the GPU bounds are twice
that (K_P, K_M, K_V): the kernel divides by sqrt(bc2) before adding eps and may contract to FMA, a bounded number of roundings
per step more or fewer than torch's.  Nothing here is fitted to the kernel's output."""
import functools
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import metrics_oracle as mo  # noqa: E402

# ----------------------------------------------------------------------------------------------------------------------
# launch geometry the sizes are built around (each mirrors one line of the launch code)
# ----------------------------------------------------------------------------------------------------------------------
BLOCK = 256                     # every kernel below launches dim3(256)
ADAMW_GRID_CAP = 4096           # train.hip sq_adamw_step: `if (nb > 4096) nb = 4096;`
MSE_GRID_CAP = 1024             # train.hip: `constexpr int RED_BLOCKS = 1024;` (sq_mse_loss_grad: `if (nb > RED_BLOCKS) nb = RED_BLOCKS;`)
CAST_GRID_CAP = 2048            # elementwise.hip grid_for: `int cap = 256 * 8`
F2B_VEC = 4                     # elementwise.hip f32_to_bf16_kernel: one float4 per thread and iteration
B2F_VEC = 8                     # elementwise.hip bf16_to_f32_x8_kernel: one u32x4 (8 bf16) per thread and iteration
METRICS_BLOCK = 256             # train.hip sq_batch_metrics: `const int nb = (G + 255) / 256;`, thread = gene

ADAMW_ONE_ROUND = ADAMW_GRID_CAP * BLOCK
MSE_ONE_ROUND = MSE_GRID_CAP * BLOCK
F2B_ONE_ROUND = CAST_GRID_CAP * BLOCK * F2B_VEC
B2F_ONE_ROUND = CAST_GRID_CAP * BLOCK * B2F_VEC

GUARD = 64                                  # sentinel elements on both sides of every output
SENT32, SENT16, SENT8 = 0x7FA5C3E1, 0x7FA5, 0xA5          # NaN bit patterns (int32 / int16 views) and the scratch guard byte
SCRATCH_GUARD = 256                         # guard bytes around the scratch (keeps its 8-byte alignment)


def f32(x):
    """A hyperparameter as the C entry receives it: rounded to float32, widened to double."""
    return float(np.float32(x))


def _seed(*parts):
    s = "/".join(str(p) for p in parts)
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(s)) % 1000003


def ulp32(x):
    """Spacing of float32 at |x| (float64 array in, float64 out); 2^-149 below the normal range."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))          # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


# ----------------------------------------------------------------------------------------------------------------------
# AdamW
# ----------------------------------------------------------------------------------------------------------------------
def adamw_ref(p, g_steps, lr, b1, b2, eps, wd, grad_scale, m0=None, v0=None, step0=1):
    """torch's single-tensor AdamW (amsgrad=False, decoupled decay) in float64 over the gradients g_steps[0], g_steps[1], ...
    taken at steps step0, step0 + 1, ...  -> namespace(p, m, v, pmax, gmax): the state after the last step, the running
    max(|p_old|, |p_new|) and the running max of |g * grad_scale|."""
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p = np.asarray(p, dtype=np.float64).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, dtype=np.float64).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, dtype=np.float64).copy()
    pmax, gmax = np.abs(p), np.zeros_like(p)
    for k, g in enumerate(g_steps):
        step = step0 + k
        g = np.asarray(g, dtype=np.float64) * gs
        p = p * (1.0 - lr * wd)
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        denom = np.sqrt(v) / np.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
        pmax, gmax = np.maximum(pmax, np.abs(p)), np.maximum(gmax, np.abs(g))
    return SimpleNamespace(p=p, m=m, v=v, pmax=pmax, gmax=gmax)


def adamw_units(ref, t, lr):
    """(unit of p, of m, of v) per element, see the module docstring."""
    return t * (ulp32(ref.pmax) + f32(lr) * 2.0 ** -24), t * 2.0 ** -24 * ref.gmax, t * 2.0 ** -24 * ref.v


def in_units(got, want, unit):
    """Worst |got - want| / unit; an element whose unit is 0 must be exact, and a NaN is never within a bound (inf)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(unit > 0, d / unit, np.where(d == 0, 0.0, np.inf))
    return float(np.where(np.isnan(q), np.inf, q).max())


HYPER = {   # lr, beta1, beta2, eps, weight_decay, grad_scale
    "prod": (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0),             # the production row: weight_decay 0 and grad_scale 1, as every caller passes
    "wd0.01": (1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0),          # torch's default decay
    "wd0.1-lr0.01": (1e-2, 0.9, 0.999, 1e-8, 0.1, 1.0),
    "scale0.125": (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.125),     # an 8-rank sum: the gradients are the production row's times 8
    "beta0.5-0.9-eps1e-3": (1e-3, 0.5, 0.9, 1e-3, 0.0, 1.0),   # eps and both bias corrections matter visibly
}
ADAMW_SIZES = (1, 3, 255, 256, 257, ADAMW_ONE_ROUND, ADAMW_ONE_ROUND + 257)
TRAJ_STEPS = 12
LATE_STEPS = (1000, 100000)
BUCKET_BOUNDS = (0, 257, 1000003)           # + n: three uneven slices of the second-round size


def _adamw_case(hyper, n, step0, steps, off):
    return dict(id=f"adamw-{hyper}-n{n}-" + (f"traj{steps}" if step0 == 1 else f"step{step0}") + f"-off{off}", hyper=hyper, n=n,
                step0=step0, steps=steps, off=off)


# every size under the production row, every other row at two blocks; offsets 0..3 in turn, all of 1, 2, 3 also at the
# second-round size (the single late step there)
ADAMW_CASES = ([_adamw_case("prod", n, 1, TRAJ_STEPS, (i + 1) % 4) for i, n in enumerate(ADAMW_SIZES)] +
               [_adamw_case(h, 257, 1, TRAJ_STEPS, (i + 2) % 4) for i, h in enumerate(HYPER) if h != "prod"] +
               [_adamw_case(h, 257, s, 1, (i + j) % 4) for i, h in enumerate(HYPER) for j, s in enumerate(LATE_STEPS)] +
               [_adamw_case("prod", ADAMW_ONE_ROUND + 257, 1000, 1, 1), _adamw_case("wd0.01", ADAMW_ONE_ROUND + 257, 1000, 1, 2)])
ADAMW_BY_ID = {c["id"]: c for c in ADAMW_CASES}
BUCKET_CASE = "adamw-wd0.01-n%d-step1000-off2" % (ADAMW_ONE_ROUND + 257)


def zero_block(n):
    """Elements whose gradients and moments are exactly zero: their update is 0, p changes by decay alone."""
    return slice(n // 3, n // 3 + (n + 7) // 8) if n >= 3 else slice(0, 0)


@functools.lru_cache(maxsize=4)
def _adamw_data(n, step0, steps):
    """Shared by all hyperparameter rows of one (n, steps): p0, unscaled gradients [steps, n], m0, v0 (float32)."""
    rng = np.random.default_rng(_seed("adamw", n, step0, steps))
    p0 = np.where(rng.random(n) < 0.1, 1.0 + 0.1 * rng.standard_normal(n), 0.02 * rng.standard_normal(n)).astype(np.float32)
    mag = np.exp(rng.uniform(-12.0, 0.0, n))                        # log-uniform over 5 decades, fixed per element
    g = (rng.standard_normal((steps, n)) * mag).astype(np.float32)
    g[:, zero_block(n)] = 0.0
    if step0 == 1:
        m0 = v0 = np.zeros(n, dtype=np.float32)
    else:                                                            # |m0| <= |g|: the m unit (running max |g|) covers it
        m0 = (rng.uniform(-1.0, 1.0, n) * np.abs(g[0])).astype(np.float32)
        m0 = np.clip(m0, -np.abs(g[0]), np.abs(g[0]))
        v0 = (g[0].astype(np.float64) ** 2 * rng.uniform(0.25, 4.0, n)).astype(np.float32)
    for a in (p0, g, m0, v0):
        a.setflags(write=False)
    return p0, g, m0, v0


def adamw_problem(case):
    """-> namespace(case, hyper (float32 values widened), p0, g [steps, n] as handed to the entry, m0, v0, t, zero)."""
    p0, g, m0, v0 = _adamw_data(case["n"], case["step0"], case["steps"])
    h = tuple(f32(x) for x in HYPER[case["hyper"]])
    if h[5] != 1.0:
        g = (g / np.float32(h[5])).astype(np.float32)               # 1 / 0.125 = 8: exact, and g * 8 * 0.125 == g
    return SimpleNamespace(case=case, hyper=h, p0=p0, g=g, m0=m0, v0=v0, t=case["steps"], zero=zero_block(case["n"]))


@functools.lru_cache(maxsize=4)
def adamw_expect(case_id):
    """The float64 reference of one case (shared, do not modify) and its three units."""
    c = ADAMW_BY_ID[case_id]
    q = adamw_problem(c)
    ref = adamw_ref(q.p0, q.g, *q.hyper, m0=q.m0, v0=q.v0, step0=c["step0"])
    return ref, adamw_units(ref, q.t, q.hyper[0])


def decay_candidates(p0, lr, wd, steps):
    """What `p *= (1.0f - lr * wd)` leaves of float32 p0 after `steps` steps when the update is 0: with the factor rounded
    twice (product, then difference) and with the factor as one fused multiply-add, which a compiler may choose.  Both are
    correctly rounded float32 evaluations of the same expression; the two factors differ by at most one ulp."""
    lr32, wd32 = np.float32(lr), np.float32(wd)
    f_two = np.float32(1.0) - lr32 * wd32
    f_fma = np.float32(1.0 - float(lr32) * float(wd32))             # the double product of two floats is exact
    out = []
    for f in (f_two, f_fma):
        p = p0.astype(np.float32).copy()
        for _ in range(steps):
            p = p * f
        out.append(p)
    return out


def adamw_torch(case, double_hyper=False):
    """torch.optim.AdamW(foreach=False) on CPU float32 over the case -> (p, m, v) as float64 arrays.  Hyperparameters: the
    float32 values widened (the reference's), or with double_hyper the decimal doubles a Python caller would write."""
    q = adamw_problem(case)
    lr, b1, b2, eps, wd, gs = HYPER[case["hyper"]] if double_hyper else q.hyper
    p = torch.nn.Parameter(torch.from_numpy(q.p0.copy()))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=False, foreach=False)
    if case["step0"] != 1:
        opt.state[p] = {"step": torch.tensor(float(case["step0"] - 1)), "exp_avg": torch.from_numpy(q.m0.copy()),
                        "exp_avg_sq": torch.from_numpy(q.v0.copy())}
    for k in range(q.t):
        p.grad = torch.from_numpy(q.g[k] * np.float32(gs))
        opt.step()
    st = opt.state[p]
    return p.detach().numpy().astype(np.float64), st["exp_avg"].numpy().astype(np.float64), st["exp_avg_sq"].numpy().astype(np.float64)


def adamw_emulate(case, mistake=None):
    """The kernel's own operation order in NumPy float32 without FMA (csrc/train.hip adamw_kernel; step_size and bc2_sqrt
    from double on the host, as sq_adamw_step forms them) -> (p, m, v) float32.  `mistake` restates one value-only bug:
      no_decay      the weight-decay line is missing
      sqrt_of_ratio sqrtf(v / bc2) + eps  in place of  sqrtf(v) / sqrt(bc2) + eps: the same real number, other roundings
      no_grad_scale grad_scale ignored
      no_eps        sqrtf(v) / sqrt(bc2)  without  + eps
      eps_first     (sqrtf(v) + eps) / sqrt(bc2): eps added before the bias correction
      swapped_betas beta1 and beta2 exchanged
      no_bc1        step_size = lr (first bias correction missing)"""
    q = adamw_problem(case)
    lr, b1, b2, eps, wd, gs = (np.float32(x) for x in q.hyper)
    if mistake == "swapped_betas":
        b1, b2 = b2, b1
    one = np.float32(1.0)
    p, m, v = q.p0.copy(), q.m0.copy(), q.v0.copy()
    for k in range(q.t):
        step = case["step0"] + k
        bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
        step_size = np.float32(float(lr) if mistake == "no_bc1" else float(lr) / bc1)
        bc2_sqrt = np.float32(np.sqrt(bc2))
        g = q.g[k] if mistake == "no_grad_scale" else q.g[k] * gs
        if mistake != "no_decay":
            p = p * (one - lr * wd)
        m = m + (g - m) * (one - b1)
        v = v * b2 + (one - b2) * g * g
        if mistake == "sqrt_of_ratio":
            denom = np.sqrt(v / (bc2_sqrt * bc2_sqrt)) + eps
        elif mistake == "eps_first":
            denom = (np.sqrt(v) + eps) / bc2_sqrt
        else:
            denom = np.sqrt(v) / bc2_sqrt + (np.float32(0) if mistake == "no_eps" else eps)
        with np.errstate(invalid="ignore", divide="ignore"):        # no_eps: 0 / 0 in the zero block
            p = p - step_size * (m / denom)
    return p, m, v


# worst deviation of torch's CPU float32 AdamW from adamw_ref over ADAMW_CASES, in the units above, rounded up
# (tests/test_train_prim_host.py::test_torch_fp32_adamw_in_units_of_the_reference measures it and holds this record to it)
# measured: p 2.408, m 0.997, v 1.978 (the single late steps; the 12-step trajectories stay below 0.7 of their t-fold unit)
TORCH_UNITS = dict(p=2.6, m=1.1, v=2.1)
K_P, K_M, K_V = (2.0 * TORCH_UNITS[k] for k in ("p", "m", "v"))


# ----------------------------------------------------------------------------------------------------------------------
# MSE loss and gradient
# ----------------------------------------------------------------------------------------------------------------------
def mse_ref(pred, target, scale):
    """-> (grad float32, loss float64).  d = pred - target and grad = scale * d are float32 operations of the entry itself."""
    d = pred.astype(np.float32) - target.astype(np.float32)
    grad = np.float32(scale) * d
    return grad, float(np.sum(d.astype(np.float64) ** 2) / d.size)


MSE_SIZES = (1, 255, 257, MSE_ONE_ROUND, MSE_ONE_ROUND + 1, 3 * 2 ** 18 + 5)
ONEHOT_AT = (0, 255, 256, 262143, 262144, -1)
ONEHOT_D = 0.75
MSE_LOSS_RTOL = 2.0 ** -22
_SCALES = ("2/n", 0.37, -3.0, 1.0 / 3.0, 1.0, 1e-4)


def _mse_cases():
    cases, k = [], 0
    for n in MSE_SIZES:
        for kind in ("random", "large"):
            cases.append(dict(id=f"mse-{kind}-n{n}", n=n, kind=kind, at=None, scale=_SCALES[k % len(_SCALES)]))
            k += 1
        for at in sorted({a % n for a in ONEHOT_AT if a < n}):
            cases.append(dict(id=f"mse-onehot-n{n}-at{at}", n=n, kind="onehot", at=at, scale=_SCALES[k % len(_SCALES)]))
            k += 1
    # a thread's first element has d = 1, its seven or eight later ones d^2 just under 2^-24: a float32 accumulator stays at 1
    cases.append(dict(id=f"mse-stagnation-n{STAGNATION_N}", n=STAGNATION_N, kind="stagnation", at=None, scale=0.37))
    return cases


STAGNATION_N = 8 * MSE_ONE_ROUND + 5
STAGNATION_D = float(np.float32(np.sqrt(0.98 * 2.0 ** -24)))
MSE_CASES = _mse_cases()
MSE_BY_ID = {c["id"]: c for c in MSE_CASES}


@functools.lru_cache(maxsize=4)
def mse_problem(case_id):
    """-> namespace(pred, target (float32), scale (python float), grad_ref float32, loss_ref float64); shared, read-only."""
    c = MSE_BY_ID[case_id]
    n = c["n"]
    rng = np.random.default_rng(_seed("mse", n, c["kind"]))
    if c["kind"] == "random":
        target = (rng.random(n) * 8).astype(np.float32)
        pred = (target + rng.standard_normal(n)).astype(np.float32)
    elif c["kind"] == "large":                                       # values near 1e4, differences near 1e-3
        target = (1e4 + rng.standard_normal(n)).astype(np.float32)
        pred = (target.astype(np.float64) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    elif c["kind"] == "stagnation":
        target = np.zeros(n, dtype=np.float32)
        pred = np.full(n, STAGNATION_D, dtype=np.float32)
        pred[:MSE_ONE_ROUND] = 1.0
    else:
        target = (rng.random(n) * 8).astype(np.float32)
        pred = target.copy()
        pred[c["at"]] = target[c["at"]] + np.float32(ONEHOT_D)
    scale = 2.0 / n if c["scale"] == "2/n" else c["scale"]
    grad, loss = mse_ref(pred, target, scale)
    for a in (pred, target, grad):
        a.setflags(write=False)
    return SimpleNamespace(case=c, n=n, pred=pred, target=target, scale=scale, grad_ref=grad, loss_ref=loss)


# ----------------------------------------------------------------------------------------------------------------------
# batch metrics
# ----------------------------------------------------------------------------------------------------------------------
def metrics_ref(pred, target):
    """-> (MAE, mean Pearson r over the genes used, number of genes used), float64: oracle/metrics_oracle.py's
    mean_absolute_error and compute_correlations_vectorised; the count restates the latter's two filters."""
    mae = mo.mean_absolute_error(target, pred)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r_mean = float(mo.compute_correlations_vectorised(target, pred))
    r = column_r(pred, target)
    return mae, r_mean, int(np.count_nonzero(~np.isnan(r)))


def column_r(pred, target):
    """Per-gene r in float64, NaN for a gene that does not enter the mean (constant target, or NaN r)."""
    y, p = target.astype(np.float64), pred.astype(np.float64)
    yc, pc = y - y.mean(0), p - p.mean(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (yc * pc).sum(0) / np.sqrt((yc * yc).sum(0) * (pc * pc).sum(0))
    r[~(y != y[0:1]).any(0)] = np.nan
    return r


METRICS_G = (1, 255, 256, 257, 513)
METRICS_B = (1, 2, 3, 64)
KINDS = ("ord", "const_t", "const_p", "pos1", "neg1", "offset")
VALID_KINDS = ("ord", "pos1", "neg1", "offset")
MIN_SPREAD = 1e-3               # a valid column's standard deviation over |mean|, both arrays ...
MIN_SPREAD_OFFSET = 5e-5        # ... except the large-offset kind, which is mean 1e4, deviation 1 by construction (1e-4)
METRICS_MAE_RTOL = 2.0 ** -22
METRICS_R_ATOL = 1e-6           # tests/test_gpu_train.py


def _metrics_cases():
    cases = [dict(id=f"metrics-mixed-B{B}-G{G}", B=B, G=G, layout="mixed", at=None) for G in METRICS_G for B in METRICS_B]
    for G in METRICS_G:
        for at in sorted({a for a in (0, 255, 256, G - 1) if a < G}):
            cases.append(dict(id=f"metrics-one-valid-B{3 if at % 2 else 64}-G{G}-at{at}", B=3 if at % 2 else 64, G=G, layout="one", at=at))
        cases.append(dict(id=f"metrics-none-valid-B3-G{G}", B=3, G=G, layout="none", at=None))
    return cases


METRICS_CASES = _metrics_cases()
METRICS_BY_ID = {c["id"]: c for c in METRICS_CASES}


def metrics_kinds(case):
    G = case["G"]
    if case["layout"] == "mixed":                                   # every kind in every block of 256 genes, the block edges varied
        return ["ord"] if G == 1 else [KINDS[(5 * g + g // 256 + G) % 6] for g in range(G)]
    kinds = [("const_t", "const_p")[g % 2] for g in range(G)]
    if case["layout"] == "one":
        kinds[case["at"]] = "ord"
    return kinds


def _unit_rows(rng, B, G):
    """[B, G] with every column at mean 0, standard deviation 1 (all zero for B = 1)."""
    z = rng.standard_normal((B, G))
    z = z - z.mean(0)
    s = z.std(0)
    return z / np.where(s > 0, s, 1.0)


@functools.lru_cache(maxsize=4)
def metrics_problem(case_id):
    """-> namespace(pred, target float32 [B, G], kinds, n_valid, mae, r, count (the float64 reference)); shared, read-only."""
    c = METRICS_BY_ID[case_id]
    B, G = c["B"], c["G"]
    rng = np.random.default_rng(_seed("metrics", case_id))
    kinds = metrics_kinds(c)
    z, w = _unit_rows(rng, B, G), _unit_rows(rng, B, G)
    mix = 0.6 * z + 0.8 * w
    sd = mix.std(0)
    mix = mix / np.where(sd > 0, sd, 1.0)                           # unit deviation again: r(z, mix) stays what the weights made it
    target = rng.uniform(1.0, 8.0, G) + rng.uniform(0.5, 2.0, G) * z
    pred = rng.uniform(1.0, 8.0, G) + rng.uniform(0.5, 2.0, G) * mix
    const = rng.uniform(1.0, 8.0, G)
    ints = np.stack([rng.permutation(B) for _ in range(G)], axis=1) + rng.integers(-4, 5, G)      # small integers, all distinct per column
    for g, kind in enumerate(kinds):
        if kind == "const_t":
            target[:, g] = const[g]
        elif kind == "const_p":
            pred[:, g] = const[g]
        elif kind in ("pos1", "neg1"):                              # an affine image, exact in float32: r = +-1
            target[:, g] = ints[:, g]
            pred[:, g] = (2.0 if kind == "pos1" else -2.0) * ints[:, g] + 3.0
        elif kind == "offset":
            target[:, g] = 1e4 + z[:, g]
            pred[:, g] = 1e4 + mix[:, g]
    pred, target = pred.astype(np.float32), target.astype(np.float32)
    mae, r, count = metrics_ref(pred, target)
    n_valid = sum(k in VALID_KINDS for k in kinds) if B > 1 else 0
    for a in (pred, target):
        a.setflags(write=False)
    return SimpleNamespace(case=c, B=B, G=G, pred=pred, target=target, kinds=kinds, n_valid=n_valid, mae=mae, r=r, count=count)


# ----------------------------------------------------------------------------------------------------------------------
# casts
# ----------------------------------------------------------------------------------------------------------------------
F2B_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1027)
F2B_BIG = F2B_ONE_ROUND + 3                 # a second grid-stride round plus a tail
F2B_SRC_OFFS, F2B_DST_OFFS = range(4), range(4)
B2F_SIZES = (0, 1, 7, 8, 9, 15, 16, 17)
B2F_BIG = B2F_ONE_ROUND + 9
B2F_SRC_OFFS, B2F_DST_OFFS = range(8), range(4)

_SPECIAL_BITS = (0x00000000, 0x80000000,                                                    # +-0
                 0x00000001, 0x80000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x80018000, 0x007FFFFF, 0x807FFFFF,  # subnormals
                 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,                                         # smallest normal; largest finite -> +-inf
                 0x7F800000, 0xFF800000,                                                     # +-inf
                 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7FBFFFFF, 0x7F808000, 0x7FFF8000)   # NaNs


@functools.lru_cache(maxsize=1)
def f2b_values():
    """int32 bit patterns: for each upper half h the floats just below, on and just above the tie between h and h + 1, then
    the special values.  NaN inputs are included (their result must be a NaN)."""
    h = np.arange(65536, dtype=np.uint32) << 16
    bits = np.concatenate([h | 0x7FFF, h | 0x8000, h | 0x8001, np.array(_SPECIAL_BITS, dtype=np.uint32)])
    bits = bits.view(np.int32)
    bits.setflags(write=False)
    return bits


def f2b_expect(bits_i32):
    """torch's CPU float32 -> bfloat16 of the given bit patterns -> (int16 bit patterns, mask of NaN inputs)."""
    x = torch.from_numpy(np.array(bits_i32, dtype=np.int32)).view(torch.float32)
    return x.to(torch.bfloat16).view(torch.int16).numpy(), torch.isnan(x).numpy()


def rne_bits(bits_i32):
    """Independent integer round-to-nearest-even of float32 bit patterns to bf16 (add 0x7fff + lsb, shift); not for NaN."""
    u = np.asarray(bits_i32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16).view(np.int16)


def f2b_sample(n, salt):
    """n patterns drawn from f2b_values (ties, specials and NaNs among them), reproducibly."""
    v = f2b_values()
    return v[np.random.default_rng(_seed("f2b", n, salt)).integers(0, v.size, n)]


def b2f_patterns():
    return np.arange(65536, dtype=np.uint16).view(np.int16)


def b2f_expect(bits_i16):
    """pattern << 16 as int32 bit patterns; the host test holds torch's .float() to it."""
    return (np.asarray(bits_i16).view(np.uint16).astype(np.uint32) << 16).view(np.int32)


def b2f_sample(n, salt):
    return np.random.default_rng(_seed("b2f", n, salt)).integers(0, 65536, n).astype(np.uint16).view(np.int16)
