"""Is every row of tests/gemm_cases.py a fair test?  (CPU only.)

The GPU sweep (test_gpu_gemm_contract.py) holds sq_linear and the weight-gradient entries to the tolerances of
tests/test_gpu_gemm.py against float64.  That only means something if a correct implementation in the row's own arithmetic sits
comfortably inside the bound at the row's operands, if the rows reach the branches they name, and if the bound and the
sentinels would catch the mistakes the rows are there for.

* Conditioning: the plain torch float32 product of the same (bf16-exact) operands, float32 epilogue, is within a QUARTER of the
  row's tolerance of the float64 reference, and touches no sentinel.  A bf16-output row is held to that on the float32 result
  before the output rounding; after the rounding it is held to the tolerance itself: rounding to bf16 (8 significant bits) alone moves an element
  of the largest element's binade [2^e, 2^(e+1)) by up to 2^(e-8), i.e. by 2^-9 .. 2^-8 = 2.0e-3 .. 3.9e-3 of the largest one
  (wherever in its binade that lies), which no choice of operands brings under a quarter of 5e-3 = 1.25e-3.
* Coverage: ids are unique, every branch the sweep was asked to reach has a row, and the branch rows reach their branch by the
  launch rule (gemm_cases.nt_dispatch restates csrc/gemm.hip launch_t).
* Teeth: seven kernel mistakes, restated as numpy / torch emulations, each push their target row past ten times its tolerance
  or change a sentinel bit."""
import pytest
import torch

import gemm_cases as gc

NT_PARAMS = [(r, d) for r in gc.NT_ALL for d in gc.nt_dtypes(r)]
NT_IDS = [f"{r['id']}-{d}" for r, d in NT_PARAMS]


def _assert_conditioned(p, what):
    err, touched = gc.judge(gc.emulate_nt(p), p.idx, p.ref)
    assert touched == 0, what
    if p.out == "bf16":
        pre = gc.prerounding_error(p)
        assert pre < p.tol / 4 and err < p.tol, (what, pre, err)
        return pre
    assert err < p.tol / 4, (what, err, p.tol)
    return err


@pytest.mark.parametrize("row,dtype", NT_PARAMS, ids=NT_IDS)
def test_nt_rows_are_well_conditioned(row, dtype):
    if row["family"] == "epi":
        worst = max(_assert_conditioned(gc.nt_problem(row, dtype, **v), v) for v in gc.EPI_PRODUCT)
    else:
        worst = _assert_conditioned(gc.nt_problem(row, dtype), row["id"])
    print(f"float32 torch product vs float64, {row['id']} {dtype}: {worst:.2e} (tolerance {gc.nt_tol(dtype, row):.0e})")


@pytest.mark.parametrize("row", gc.TN_CASES + gc.GROUP_CASES, ids=lambda r: r["id"])
def test_tn_rows_are_well_conditioned(row):
    for member in range(row.get("members", 1)):
        p = gc.tn_problem(row, member)
        dw, db = gc.emulate_tn(p)
        e_dw, t_dw = gc.judge(dw, p.idx, p.ref_dw)
        e_db, t_db = gc.judge(db, p.db_idx, p.ref_db)
        print(f"float32 torch product vs float64, {row['id']} member {member}: dW {e_dw:.2e} dbias {e_db:.2e}")
        assert t_dw == 0 and t_db == 0
        assert e_dw < p.tol / 4 and e_db < p.tol / 4, (e_dw, e_db)


def test_ids_are_unique_and_every_named_branch_has_a_row():
    for table, required in ((gc.NT_ALL, gc.NT_REQUIRED_TAGS), (gc.TN_CASES, gc.TN_REQUIRED_TAGS), (gc.GROUP_CASES, gc.GROUP_REQUIRED_TAGS)):
        ids = [r["id"] for r in table]
        assert len(set(ids)) == len(ids)
        have = {t for r in table for t in r["tags"]}
        missing = [t for t in required if t not in have]
        assert not missing, missing
        assert all(r["branch"] for r in table)
    # every stride and tiny row runs under the rule and under the four forced tiles; both dtypes wherever K allows
    assert all(len(gc.nt_dtypes(r)) == 2 for r in gc.NT_STRIDE)
    for k in ("epc", "2epc", 32, 64, 72):
        assert any(r["K"] == k and len(gc.nt_dtypes(r)) == 2 for r in gc.NT_TINY), k
    # the epilogue product is the full one: dtype (both epi shapes in both dtypes) x bias x residual x act x out
    assert len(gc.EPI_PRODUCT) == 2 * 3 * 3 * 2
    assert {d for r in gc.NT_EPI if "epi-scalar" in r["tags"] for d in gc.nt_dtypes(r)} == {"f32", "bf16"}
    assert len(gc.TN_DY_PAD_NAN["tags"]) and gc.tn_problem(gc.TN_DY_PAD_NAN).dY_buf[:40, 9:16].isnan().all()


def test_branch_rows_reach_their_branch_by_the_launch_rule():
    for r in gc.NT_BRANCH:
        for d in gc.nt_dtypes(r):
            got = gc.nt_dispatch(d, r["M"], r["N"], gc.nt_k(r, d))
            assert got["tile"] == r["want_tile"] and got["splitk"] == 1, (r["id"], d, got)
            assert gc.nt_k(r, d) < 512                      # neither gemm_p8.hip nor the ring kernel (both need K >= 512)
        if r.get("want_one_buffer"):
            assert gc.nt_dispatch("f32", r["M"], r["N"], r["K"])["one_buffer"]
    by = gc.NT_BY_ID
    for d in ("f32", "bf16"):
        r = by["nt-split-forced-empty-slice"]
        got = gc.nt_dispatch(d, r["M"], r["N"], gc.nt_k(r, d), r["ws"], r["split"])
        assert got["nk"] == 5 and got["splitk"] == 4 and gc.last_slice_is_empty(got["nk"], got["splitk"])
        r = by["nt-split-n-not-multiple-of-8"]
        assert gc.nt_dispatch(d, r["M"], r["N"], r["K"], r["ws"])["splitk"] == 1
        for rid in ("nt-split-strided-vector-reduce", "nt-split-strided-scalar-reduce"):
            r = by[rid]
            assert gc.nt_dispatch(d, r["M"], r["N"], r["K"], r["ws"])["splitk"] > 1
    r = by["nt-split-natural-empty-slice"]
    got = gc.nt_dispatch("f32", r["M"], r["N"], r["K"], r["ws"])
    assert got == dict(tile=22, splitk=5, per=4, nk=16, one_buffer=False) and gc.last_slice_is_empty(16, 5)
    r = by["nt-split-workspace-one-byte-short"]
    got = gc.nt_dispatch("f32", r["M"], r["N"], r["K"], r["ws"])
    assert got["tile"] == 22 and got["splitk"] == 1
    assert gc.nt_dispatch("f32", r["M"], r["N"], r["K"], r["ws"] + 1)["splitk"] == 2
    # weight gradients: the forced slice count leaves the last slice without a token step; the ring form takes the ring shape
    for row in gc.TN_CASES:
        for d in ("f32", "bf16"):
            nk = -(-row["T"] // (64 if d == "bf16" else 32))
            assert gc.last_slice_is_empty(nk, gc.tn_empty_slice_split(d, row["T"]))
    for row in gc.GROUP_CASES:
        ring = row["NO"] % 128 == 0 and row["NI"] % 128 == 0 and -(-row["T"] // 64) >= 8 and (row["NO"] // 128) * (row["NI"] // 128) * row["members"] >= 8
        assert ring == ("group-ring-shape" in row["tags"] and row["members"] >= 2), row["id"]


# ---- teeth: what a subtly wrong kernel would do has to show at ten times the bound, or in a sentinel ----
def _bitten(p, mistake):
    err, touched = gc.judge(gc.emulate_nt(p, mistake), p.idx, p.ref)
    print(f"{mistake} at {p.row['id']} {p.dtype}: error {err:.2e} (tolerance {p.tol:.0e}), {touched} sentinel elements changed")
    return touched > 0 or not err < 10 * p.tol


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mistake,rid", [
    ("lda_as_K", "nt-stride-ldc_N-ldres_N"),
    ("drop_last_chunk", "nt-stride-ldc_N-ldres_N"), ("drop_last_chunk", "nt-tiny-M2-N7-K2epc"), ("drop_last_chunk", "nt-tiny-M40-N12-K8"),
    ("bias_partial_chunk", "nt-tiny-M40-N12-K8"), ("bias_partial_chunk", "nt-tiny-M2-N7-K2epc"), ("bias_partial_chunk", "nt-tiny-M40-N1-K32"),
    ("res_at_ldc", "nt-stride-ldc_N-ldres_vec"), ("res_at_ldc", "nt-stride-ldc_vec-ldres_odd"),
    ("stale_slice", "nt-split-forced-empty-slice"), ("stale_slice", "nt-split-natural-empty-slice"),
    ("ldc_as_N", "nt-stride-ldc_vec-ldres_N"), ("ldc_as_N", "nt-stride-ldc_odd-ldres_N"), ("ldc_as_N", "nt-tiny-M40-N1-K32"),
])
def test_nt_mistakes_would_show(mistake, rid, dtype):
    row = gc.NT_BY_ID[rid]
    if dtype not in gc.nt_dtypes(row):
        dtype = gc.nt_dtypes(row)[0]
    p = gc.nt_problem(row, dtype)
    if mistake == "res_at_ldc":
        assert p.res == "bf16" and p.ldc != p.ldres
    assert _bitten(p, mistake)


@pytest.mark.parametrize("rid", ["tn-NO1-NI32-T40-dy0-x0-w0", "tn-NO9-NI72-T40-dy8-x0-w0-nanpad", "tn-NO65-NI136-T32-dy16-x0-w4"])
def test_dbias_summed_over_lddy_columns_would_show(rid):
    p = gc.tn_problem(gc.TN_BY_ID[rid])
    _, db = gc.emulate_tn(p, "dbias_over_lddy")
    err, touched = gc.judge(db, p.db_idx, p.ref_db)
    print(f"dbias over lddy columns at {rid}: {touched} guard elements changed")
    assert touched > 0
    _, db = gc.emulate_tn(p)
    assert gc.judge(db, p.db_idx, p.ref_db)[1] == 0
