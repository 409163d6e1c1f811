"""CPU checks of tests/train_prim_cases.py: the float64 references against torch / NumPy, the conditions on the inputs, and
what torch's own float32 AdamW loses against the float64 reference in the units the GPU test bounds the kernel in
(tests/test_gpu_train_prims.py allows twice that).  Prints `TRAIN_PRIM_HOST ...` lines with every measured figure."""
import os
import re

import numpy as np
import pytest
import torch

import train_prim_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sequoia-pub_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_grid_caps_mirror_the_launch_code():
    """The sizes are built around the launch code's caps: hold the constants to the lines they name."""
    train, elem = _source("train.hip"), _source("elementwise.hip")
    assert f"if (nb > {tc.ADAMW_GRID_CAP}) nb = {tc.ADAMW_GRID_CAP};" in train
    assert f"constexpr int RED_BLOCKS = {tc.MSE_GRID_CAP};" in train and "if (nb > RED_BLOCKS) nb = RED_BLOCKS;" in train
    assert f"const int nb = (G + {tc.METRICS_BLOCK - 1}) / {tc.METRICS_BLOCK};" in train
    m = re.search(r"inline int grid_for\(size_t work_items, int block, int cap = (\d+) \* (\d+)\)", elem)
    assert m and int(m.group(1)) * int(m.group(2)) == tc.CAST_GRID_CAP
    assert "const size_t n4 = n / 4;" in elem and tc.F2B_VEC == 4
    assert "const size_t n8 = n / 8;" in elem and tc.B2F_VEC == 8
    for kernel in ("mse_kernel", "adamw_kernel", "metrics_kernel", "f32_to_bf16_kernel", "bf16_to_f32_x8_kernel"):
        src = train if kernel in train else elem
        assert re.search(rf"hipLaunchKernelGGL\({kernel}, dim3\([^;]*?\), dim3\({tc.BLOCK}\)", src), kernel
    # the sizes: exactly one round, and a second round for some threads / a tail
    assert tc.ADAMW_ONE_ROUND in tc.ADAMW_SIZES and tc.ADAMW_ONE_ROUND + 257 in tc.ADAMW_SIZES
    assert tc.MSE_ONE_ROUND in tc.MSE_SIZES and tc.MSE_ONE_ROUND + 1 in tc.MSE_SIZES and max(tc.MSE_SIZES) > 3 * tc.MSE_ONE_ROUND
    assert tc.F2B_BIG > tc.F2B_ONE_ROUND and tc.F2B_BIG % tc.F2B_VEC and tc.B2F_BIG > tc.B2F_ONE_ROUND and tc.B2F_BIG % tc.B2F_VEC


# ----------------------------------------------------------------------------------------------------------------------
# AdamW
# ----------------------------------------------------------------------------------------------------------------------
def test_adamw_table_covers_what_it_names():
    ids = [c["id"] for c in tc.ADAMW_CASES]
    assert len(set(ids)) == len(ids) and tc.BUCKET_CASE in tc.ADAMW_BY_ID
    traj = [c for c in tc.ADAMW_CASES if c["step0"] == 1]
    assert {c["n"] for c in traj if c["hyper"] == "prod"} == set(tc.ADAMW_SIZES)
    assert {c["hyper"] for c in traj} == set(tc.HYPER) and all(c["steps"] == tc.TRAJ_STEPS for c in traj)
    for s in tc.LATE_STEPS:
        assert {c["hyper"] for c in tc.ADAMW_CASES if c["step0"] == s} == set(tc.HYPER)
    assert {c["off"] for c in tc.ADAMW_CASES} == {0, 1, 2, 3}
    assert {1, 2, 3} <= {c["off"] for c in tc.ADAMW_CASES if c["n"] > tc.ADAMW_ONE_ROUND}       # offsets in the second round too
    assert tc.BUCKET_BOUNDS[-1] < tc.ADAMW_BY_ID[tc.BUCKET_CASE]["n"] and tc.HYPER["wd0.01"][4] > 0


def test_adamw_inputs_meet_their_conditions():
    tiny = float(np.finfo(np.float32).tiny)
    for c in tc.ADAMW_CASES:
        q = tc.adamw_problem(c)
        zero = np.zeros(c["n"], dtype=bool)
        zero[q.zero] = True
        assert zero.any() == (c["n"] >= 3)
        g_eff = q.g.astype(np.float64) * q.hyper[5]
        assert np.all(g_eff[:, zero] == 0) and np.all(q.m0[zero] == 0) and np.all(q.v0[zero] == 0)
        sq = (g_eff[:, ~zero].astype(np.float32)) ** 2
        assert sq.size == 0 or float(sq.min()) >= tiny, (c["id"], "g * g underflows to a float32 subnormal")
        if c["n"] > 100:                                                                # about five decades of magnitudes
            span = np.abs(g_eff[:, ~zero])
            assert span.max() / np.median(span) > 1e2 and np.median(span) / np.quantile(span, 0.05) > 1e2, c["id"]
        assert np.all(q.v0 >= 0) and np.all(np.abs(q.m0) <= np.abs(g_eff[0]))         # the m unit covers the start moments
        if c["step0"] != 1:
            assert np.all(q.v0[~zero] > 0) and np.any(q.m0 != 0)


def test_grad_scale_row_is_the_production_row_on_scaled_gradients():
    """grad_scale = 0.125 on gradients times 8 has the production row's reference exactly (powers of two)."""
    a = next(c for c in tc.ADAMW_CASES if c["hyper"] == "prod" and c["step0"] == 1 and c["n"] == 257)
    b = next(c for c in tc.ADAMW_CASES if c["hyper"] == "scale0.125" and c["step0"] == 1 and c["n"] == 257)
    qa, qb = tc.adamw_problem(a), tc.adamw_problem(b)
    assert np.array_equal(qb.g, qa.g * np.float32(8)) and qb.hyper[5] == 0.125
    ra, rb = tc.adamw_expect(a["id"])[0], tc.adamw_expect(b["id"])[0]
    assert np.array_equal(ra.p, rb.p) and np.array_equal(ra.m, rb.m) and np.array_equal(ra.v, rb.v)


def test_torch_fp32_adamw_in_units_of_the_reference():
    """adamw_ref against torch.optim.AdamW(foreach=False) on CPU float32 (same float32-valued hyperparameters): the worst
    deviation in the three units is what TORCH_UNITS records; the GPU bound is twice that.  The kernel's operation order,
    emulated in NumPy float32, has to fit the GPU bound with room."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    emu = dict(p=0.0, m=0.0, v=0.0)
    for c in tc.ADAMW_CASES:
        ref, units = tc.adamw_expect(c["id"])
        got = dict(zip("pmv", tc.adamw_torch(c)))
        kern = dict(zip("pmv", tc.adamw_emulate(c)))
        line = []
        for k, want, unit in zip("pmv", (ref.p, ref.m, ref.v), units):
            e, ek = tc.in_units(got[k], want, unit), tc.in_units(kern[k], want, unit)
            worst[k], emu[k] = max(worst[k], e), max(emu[k], ek)
            line.append(f"{k} torch {e:.2f} emulated kernel {ek:.2f}")
        print(f"TRAIN_PRIM_HOST {c['id']}: " + ", ".join(line) + " units")
    print(f"TRAIN_PRIM_HOST adamw worst torch units: p {worst['p']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}; emulated kernel: "
          f"p {emu['p']:.3f} m {emu['m']:.3f} v {emu['v']:.3f}; recorded {tc.TORCH_UNITS}; K_P {tc.K_P} K_M {tc.K_M} K_V {tc.K_V}")
    for k in "pmv":
        assert np.isfinite(worst[k]) and worst[k] <= tc.TORCH_UNITS[k] <= 1.5 * worst[k], (k, worst[k], tc.TORCH_UNITS[k])
        assert emu[k] <= 2.0 * tc.TORCH_UNITS[k], (k, emu[k])
    assert (tc.K_P, tc.K_M, tc.K_V) == tuple(2.0 * tc.TORCH_UNITS[k] for k in "pmv")


@pytest.mark.parametrize("mistake", ["no_decay", "no_grad_scale", "no_eps", "eps_first", "swapped_betas", "no_bc1"])
def test_adamw_bounds_catch_value_mistakes(mistake):
    """Each restated kernel bug (train_prim_cases.adamw_emulate) leaves the GPU bound in at least one case."""
    caught = []
    for c in tc.ADAMW_CASES:
        if c["n"] > 1000:
            continue
        ref, units = tc.adamw_expect(c["id"])
        got = tc.adamw_emulate(c, mistake)
        e = [tc.in_units(x, want, unit) for x, want, unit in zip(got, (ref.p, ref.m, ref.v), units)]
        if e[0] > tc.K_P or e[1] > tc.K_M or e[2] > tc.K_V:
            caught.append((c["id"], [f"{x:.3g}" for x in e]))
    print(f"TRAIN_PRIM_HOST mistake {mistake}: outside the bound in {len(caught)} cases, first {caught[:1]}")
    assert caught


def test_sqrt_of_the_ratio_is_a_rounding_level_rewrite():
    """sqrtf(v / (bc2_sqrt * bc2_sqrt)) + eps is the same real number as sqrtf(v) / bc2_sqrt + eps; the two differ by about
    two float32 roundings of the denominator, i.e. by a fraction of the p unit.  No bound derived from the number format can
    tell them apart, and these do not: both orders are correct AdamW.  (eps left out or added before the division is caught:
    test_adamw_bounds_catch_value_mistakes.)"""
    worst = 0.0
    for c in tc.ADAMW_CASES:
        if c["n"] > 1000:
            continue
        ref, units = tc.adamw_expect(c["id"])
        a, b = tc.adamw_emulate(c)[0], tc.adamw_emulate(c, "sqrt_of_ratio")[0]
        worst = max(worst, tc.in_units(a.astype(np.float64), b.astype(np.float64), units[0]))
        assert tc.in_units(b, ref.p, units[0]) <= tc.K_P
    print(f"TRAIN_PRIM_HOST sqrt of the ratio against ratio of the sqrt: p differs by at most {worst:.2f} units (K_P {tc.K_P})")
    assert worst < tc.K_P / 2


def test_float_hyperparameters_lower_the_second_moment_against_torch_with_doubles():
    """The documented consequence of the float ABI: 1 - 0.999f is about 1.3e-5 relative below 1 - 0.999, and so is exp_avg_sq
    against torch run with the Python doubles; the parameters move by less than their unit."""
    c = next(c for c in tc.ADAMW_CASES if c["id"].startswith("adamw-prod-n257-traj"))
    ref, units = tc.adamw_expect(c["id"])
    p, _, v = tc.adamw_torch(c, double_hyper=True)
    nz = ref.v > 0
    ratio = ref.v[nz] / v[nz]
    dp = tc.in_units(p, ref.p, units[0])
    print(f"TRAIN_PRIM_HOST float hyperparameters: exp_avg_sq(reference) / exp_avg_sq(torch, double hyperparameters) - 1 in "
          f"[{ratio.min() - 1:.3e}, {ratio.max() - 1:.3e}]; (1 - 0.999f) / (1 - 0.999) - 1 = {(1 - tc.f32(0.999)) / (1 - 0.999) - 1:.3e}; "
          f"p against torch with doubles: {dp:.2f} units")
    assert -1.6e-5 < ratio.min() - 1 and ratio.max() - 1 < -1.0e-5
    assert dp <= tc.K_P


def test_decay_candidates_differ_by_rounding_only():
    p0 = np.linspace(-2, 2, 1001).astype(np.float32)
    for lr, wd in ((1e-3, 0.01), (1e-2, 0.1), (1e-3, 0.0)):
        a, b = tc.decay_candidates(p0, lr, wd, 12)
        assert np.all(np.abs(a.astype(np.float64) - b) <= 12 * tc.ulp32(p0)), (lr, wd)
        if wd == 0.0:
            assert np.array_equal(a, p0) and np.array_equal(b, p0)
        else:
            assert np.all(np.abs(a[p0 != 0]) < np.abs(p0[p0 != 0]))


# ----------------------------------------------------------------------------------------------------------------------
# MSE
# ----------------------------------------------------------------------------------------------------------------------
def test_mse_table_and_reference():
    ids = [c["id"] for c in tc.MSE_CASES]
    assert len(set(ids)) == len(ids) and {c["n"] for c in tc.MSE_CASES} == set(tc.MSE_SIZES) | {tc.STAGNATION_N}
    assert len({c["scale"] for c in tc.MSE_CASES}) >= 4                                  # arbitrary grad_scale, not only 2 / n
    for n in tc.MSE_SIZES:
        want = {a % n for a in tc.ONEHOT_AT if a < n}
        assert {c["at"] for c in tc.MSE_CASES if c["n"] == n and c["kind"] == "onehot"} == want and n - 1 in want
    assert {c["at"] for c in tc.MSE_CASES if c["n"] == max(tc.MSE_SIZES) and c["kind"] == "onehot"} == {0, 255, 256, 262143, 262144, max(tc.MSE_SIZES) - 1}
    for c in tc.MSE_CASES:
        q = tc.mse_problem(c["id"])
        assert q.pred.shape == q.target.shape == q.grad_ref.shape == (c["n"],) and q.grad_ref.dtype == np.float32
        d = q.pred - q.target                                                           # float32
        want = float(torch.nn.MSELoss()(torch.from_numpy(d.astype(np.float64)), torch.zeros(c["n"], dtype=torch.float64)))
        assert abs(q.loss_ref - want) <= 1e-12 * want, c["id"]                          # two float64 summation orders
        if c["kind"] == "onehot":
            assert 0 <= c["at"] < c["n"] and np.count_nonzero(d) == 1 and d[c["at"]] != 0
            assert q.loss_ref == float(d[c["at"]]) ** 2 / c["n"] and np.count_nonzero(q.grad_ref) == 1
        elif c["kind"] == "stagnation":
            # per-thread accumulation in float32 (thread i takes i, i + one round, ...) leaves the bound; in double it does not
            rounds = -(-c["n"] // tc.MSE_ONE_ROUND)
            acc = np.zeros(tc.MSE_ONE_ROUND, dtype=np.float32)
            for k in range(rounds):
                part = d[k * tc.MSE_ONE_ROUND:(k + 1) * tc.MSE_ONE_ROUND]
                acc[:part.size] += part * part
            lossy = float(acc.astype(np.float64).sum() / c["n"])
            print(f"TRAIN_PRIM_HOST {c['id']}: float32 accumulators lose {abs(lossy - q.loss_ref) / q.loss_ref:.2e} (bound {tc.MSE_LOSS_RTOL:.2e})")
            assert rounds == 9 and abs(lossy - q.loss_ref) > 1.5 * tc.MSE_LOSS_RTOL * q.loss_ref
        elif c["kind"] == "large":
            assert np.abs(q.target).min() > 9e3 and np.abs(d).max() < 1e-2 and (c["n"] < 255 or np.abs(d).max() > 1e-3)
            # the float32 subtraction is part of the operation: against float64 operands the loss differs visibly
        else:
            full = float(torch.nn.MSELoss()(torch.from_numpy(q.pred.astype(np.float64)), torch.from_numpy(q.target.astype(np.float64))))
            assert abs(q.loss_ref - full) <= 1e-6 * full


# ----------------------------------------------------------------------------------------------------------------------
# metrics
# ----------------------------------------------------------------------------------------------------------------------
def test_metrics_table_and_reference():
    ids = [c["id"] for c in tc.METRICS_CASES]
    assert len(set(ids)) == len(ids)
    assert {(c["B"], c["G"]) for c in tc.METRICS_CASES if c["layout"] == "mixed"} == {(b, g) for b in tc.METRICS_B for g in tc.METRICS_G}
    for G in tc.METRICS_G:
        assert {c["at"] for c in tc.METRICS_CASES if c["layout"] == "one" and c["G"] == G} == {a for a in (0, 255, 256, G - 1) if a < G}
        assert any(c["layout"] == "none" and c["G"] == G for c in tc.METRICS_CASES)
    for c in tc.METRICS_CASES:
        q = tc.metrics_problem(c["id"])
        if c["layout"] == "mixed" and c["G"] >= 255:
            assert set(q.kinds) == set(tc.KINDS)
        y, p = q.target.astype(np.float64), q.pred.astype(np.float64)
        used, rs = 0, []
        for g, kind in enumerate(q.kinds):
            valid = kind in tc.VALID_KINDS and c["B"] > 1
            if valid:                                                                    # well spread in both arrays
                floor = tc.MIN_SPREAD_OFFSET if kind == "offset" else tc.MIN_SPREAD
                for col in (y[:, g], p[:, g]):
                    assert col.std() >= floor * abs(col.mean()), (c["id"], g, kind)
                if kind == "offset":
                    assert abs(y[:, g].mean() - 1e4) < 1 and abs(y[:, g].std() - 1) < 0.01
            if len(np.unique(q.target[:, g])) > 1:                                       # the literal loop of he2rna.py:140-149
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = np.corrcoef(y[:, g], p[:, g])[0, 1]
                assert np.isnan(r) != valid, (c["id"], g, kind)
                if not np.isnan(r):
                    used += 1
                    rs.append(r)
                    if kind in ("pos1", "neg1"):
                        assert abs(r - (1 if kind == "pos1" else -1)) < 1e-12
            else:
                assert not valid, (c["id"], g, kind)
        assert used == q.count == q.n_valid, (c["id"], used, q.count, q.n_valid)
        if used:
            assert abs(np.mean(rs) - q.r) < 1e-12, c["id"]
        else:
            assert np.isnan(q.r), c["id"]
        assert abs(q.mae - np.abs(p - y).mean()) <= 1e-15 * q.mae
        if c["B"] == 1 or c["layout"] == "none":
            assert q.count == 0
        if c["layout"] == "one":
            assert q.count == 1 and q.kinds[c["at"]] == "ord"


# ----------------------------------------------------------------------------------------------------------------------
# casts
# ----------------------------------------------------------------------------------------------------------------------
def test_f32_to_bf16_expectation_is_round_to_nearest_even():
    bits = tc.f2b_values()
    assert bits.size == 3 * 65536 + len(tc._SPECIAL_BITS)
    want, nan = tc.f2b_expect(bits)
    assert np.array_equal(want[~nan], tc.rne_bits(bits[~nan]))
    w16 = want.view(np.uint16)
    assert np.all((w16[nan] & 0x7F80) == 0x7F80) and np.all((w16[nan] & 0x007F) != 0)     # NaN in, NaN out
    assert 30 < nan.sum() < bits.size // 100 * 2
    u = bits.view(np.uint32)
    look = lambda b: int(w16[np.flatnonzero(u == b)[0]])
    assert look(0x7F7FFFFF) == 0x7F80 and look(0xFF7FFFFF) == 0xFF80                      # the largest finite float -> +-inf
    assert look(0x00008000) == 0x0000 and look(0x00018000) == 0x0002 and look(0x00008001) == 0x0001     # subnormal ties to even
    assert look(0x3F808000) == 0x3F80 and look(0x3F818000) == 0x3F82 and look(0x3F807FFF) == 0x3F80 and look(0x3F808001) == 0x3F81
    assert look(0x80000000) == 0x8000 and look(0x7F800000) == 0x7F80
    for n in tc.F2B_SIZES:
        assert tc.f2b_sample(n, 0).size == n


def test_bf16_to_f32_expectation_and_round_trip():
    pat = tc.b2f_patterns()
    want = tc.b2f_expect(pat)
    t = torch.from_numpy(pat.copy()).view(torch.bfloat16)
    assert np.array_equal(t.float().view(torch.int32).numpy(), want)
    back, nan = tc.f2b_expect(want)
    assert np.array_equal(back[~nan], pat[~nan]) and nan.sum() == 2 * 127


def test_cast_size_and_offset_tables_reach_both_sides_of_every_branch():
    assert set(tc.F2B_SIZES) >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1027} and list(tc.F2B_SRC_OFFS) == list(tc.F2B_DST_OFFS) == [0, 1, 2, 3]
    assert set(tc.B2F_SIZES) >= {0, 1, 7, 8, 9, 15, 16, 17} and list(tc.B2F_SRC_OFFS) == list(range(8)) and list(tc.B2F_DST_OFFS) == [0, 1, 2, 3]
    # with 16-byte aligned allocations and guards of GUARD elements the offsets alone decide the alignment branch
    assert tc.GUARD >= 64 and tc.GUARD * 2 % 16 == 0 and tc.GUARD * 4 % 16 == 0 and tc.SCRATCH_GUARD % 8 == 0
    f2b_vector = [(s, d) for s in tc.F2B_SRC_OFFS for d in tc.F2B_DST_OFFS if s * 4 % 16 == 0 and d * 2 % 8 == 0]
    b2f_vector = [(s, d) for s in tc.B2F_SRC_OFFS for d in tc.B2F_DST_OFFS if s * 2 % 16 == 0 and d * 4 % 16 == 0]
    assert f2b_vector == [(0, 0)] and b2f_vector == [(0, 0)]
