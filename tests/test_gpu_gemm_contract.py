"""sq_linear, sq_linear_weight_grad and sq_linear_weight_grad_group across the strides, tiny extents, dtype mixes and dispatch
branches of tests/gemm_cases.py, against float64.  Every operand buffer is padded with NaN, every output buffer is
over-allocated and filled with a sentinel bit pattern: an over-read poisons the result, a stray store changes a sentinel
(gemm_cases.judge).  tests/test_gemm_cases_host.py shows on the CPU that a correct float32 implementation uses at most a quarter
of each bound at these operands, so a failure here is the kernel's.

Every run prints `GEMM_CONTRACT <id> <dtype> ...` with the observed error; the last test prints the worst error per family and
dtype (profiles/gemm_contract_errors.txt is that output)."""
import ctypes
import time
from types import SimpleNamespace

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

from sequoia_pub_amd import _lib  # noqa: E402

CODE = {"f32": _lib.SQ_F32, "bf16": _lib.SQ_BF16}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
ESZ = {"f32": 4, "bf16": 2}
WORST = {}
T0 = time.time()
VP = ctypes.c_void_p


def _note(family, dtype, err, tol):
    WORST[(family, dtype, tol)] = max(WORST.get((family, dtype, tol), 0.0), err)


@pytest.fixture(scope="module")
def ws():
    _lib.require_gpu()
    return torch.empty(gc.WS64, dtype=torch.uint8, device="cuda")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _dev(p):
    return SimpleNamespace(A=p.A_buf.to("cuda", TORCH[p.dtype]), W=p.W_buf.to("cuda", TORCH[p.dtype]),
                           bias=p.bias.cuda() if p.bias is not None else None,
                           res=p.res_buf.to("cuda", TORCH[p.res]) if p.res_buf is not None else None)


def _linear(p, d, ws=None, ws_bytes=0):
    """One sq_linear call on the row's padded buffers into a fresh sentinel-filled output; the whole output buffer on the host."""
    C = gc.sentinel(p.c_len, p.out).cuda()
    assert p.c_off + (p.M - 1) * p.ldc + p.N <= C.numel() and p.a0 + (p.M - 1) * p.lda + p.K <= d.A.numel()
    assert p.w0 + (p.N - 1) * p.ldw + p.K <= d.W.numel() and (d.res is None or (p.M - 1) * p.ldres + p.N <= d.res.numel())
    _lib.check(_lib.lib().sq_linear(CODE[p.dtype], VP(d.A.data_ptr() + p.a0 * ESZ[p.dtype]), p.lda, VP(d.W.data_ptr() + p.w0 * ESZ[p.dtype]), p.ldw,
                                    _lib.ptr(d.bias), _lib.ptr(d.res), p.ldres, CODE[p.res] if d.res is not None else _lib.SQ_F32, p.act,
                                    VP(C.data_ptr() + p.c_off * ESZ[p.out]), CODE[p.out], p.ldc, p.M, p.N, p.K,
                                    _lib.ptr(ws) if ws_bytes else None, ws_bytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return C.cpu()


def _check_all(failures):
    assert not failures, failures


@pytest.mark.parametrize("row", gc.NT_STRIDE + gc.NT_TINY, ids=lambda r: r["id"])
def test_nt_strides_and_tiny_extents_under_the_rule_and_every_forced_tile(row):
    """Padded lda / ldw, sub-views of A, W and C, ldc and ldres chosen independently, and the smallest extents (the HE2RNA
    layers=[1] pair among them) under auto dispatch and under sq_dbg_set(0, t) for t in 11, 12, 21, 22: all five against float64."""
    _lib.require_gpu()
    lib = _lib.lib()
    failures = []
    for dtype in gc.nt_dtypes(row):
        p = gc.nt_problem(row, dtype)
        d = _dev(p)
        first = None
        try:
            for tile in (0,) + gc.FORCED_TILES:
                lib.sq_dbg_set(0, tile)
                flat = _linear(p, d)
                err, touched = gc.judge(flat, p.idx, p.ref)
                first = flat if first is None else first
                same = bool(torch.equal(_bits(flat), _bits(first)))
                print(f"GEMM_CONTRACT {row['id']} {dtype} tile {tile}: err {err:.2e} (tol {p.tol:.0e}), {touched} sentinel elements changed, "
                      f"bit-equal to the rule's tile: {same}")
                _note(row["family"], dtype, err, p.tol)
                if touched or not err < p.tol:
                    failures.append((dtype, tile, err, touched))
        finally:
            lib.sq_dbg_set(0, 0)
    _check_all(failures)


@pytest.mark.parametrize("row", gc.NT_BRANCH, ids=lambda r: r["id"])
def test_nt_dispatch_branches_reached_by_rule(row):
    """Tile 21 by both routes, tile 12 and the one-buffer LDS form, at shapes the launch rule sends there
    (test_gemm_cases_host.py holds the rows to the rule)."""
    _lib.require_gpu()
    failures = []
    for dtype in gc.nt_dtypes(row):
        p = gc.nt_problem(row, dtype)
        err, touched = gc.judge(_linear(p, _dev(p)), p.idx, p.ref)
        print(f"GEMM_CONTRACT {row['id']} {dtype}: err {err:.2e} (tol {p.tol:.0e}), {touched} sentinel elements changed")
        _note("branch", dtype, err, p.tol)
        if touched or not err < p.tol:
            failures.append((dtype, err, touched))
    _check_all(failures)


@pytest.mark.parametrize("row", gc.NT_SPLIT, ids=lambda r: r["id"])
def test_nt_split_k_empty_slices_workspace_limits_and_strided_reduce(row, ws):
    """Split-K with an empty last slice (forced and by rule), a workspace too small for two slices, N % 8 != 0 with a workspace,
    strided ldc / ldres with GELU in the reduce kernel; every row twice, bit-equal."""
    _lib.require_gpu()
    lib = _lib.lib()
    failures = []
    for dtype in gc.nt_dtypes(row):
        p = gc.nt_problem(row, dtype)
        d = _dev(p)
        lib.sq_dbg_set(2, row["split"])
        try:
            flat = _linear(p, d, ws, row["ws"])
            again = _linear(p, d, ws, row["ws"])
        finally:
            lib.sq_dbg_set(2, 0)
        err, touched = gc.judge(flat, p.idx, p.ref)
        same = bool(torch.equal(_bits(flat), _bits(again)))
        plan = gc.nt_dispatch(dtype, p.M, p.N, p.K, row["ws"], row["split"])
        print(f"GEMM_CONTRACT {row['id']} {dtype}: err {err:.2e} (tol {p.tol:.0e}), {touched} sentinel elements changed, "
              f"{plan['splitk']} slices of {plan['per']} K-tiles over {plan['nk']} by rule, second run bit-equal: {same}")
        _note("split", dtype, err, p.tol)
        if touched or not err < p.tol or not same:
            failures.append((dtype, err, touched, same))
    _check_all(failures)


@pytest.mark.parametrize("row", gc.NT_EPI, ids=lambda r: r["id"])
def test_nt_epilogue_product_of_bias_residual_activation_and_output_type(row):
    """dtype x {no bias, bias} x {no residual, f32, bf16} x {none, GELU, ReLU} x {f32, bf16 output} on the vector and on the scalar
    epilogue."""
    _lib.require_gpu()
    failures = []
    for dtype in gc.nt_dtypes(row):
        for v in gc.EPI_PRODUCT:
            p = gc.nt_problem(row, dtype, **v)
            err, touched = gc.judge(_linear(p, _dev(p)), p.idx, p.ref)
            what = f"bias {int(v['bias'])} res {v['res']} act {v['act']} out {v['out']}"
            print(f"GEMM_CONTRACT {row['id']} {dtype} {what}: err {err:.2e} (tol {p.tol:.0e}), {touched} sentinel elements changed")
            _note("epi", dtype, err, p.tol)
            if touched or not err < p.tol:
                failures.append((dtype, what, err, touched))
    _check_all(failures)


@pytest.mark.parametrize("row", gc.NT_SPECIAL, ids=lambda r: r["id"])
def test_nt_forced_p8_and_ring_kernels_with_strides(row):
    """gemm_p8.hip (tile 88, the schedules and widths test_gpu_gemm.py forces) and gemm_ring.hip (tile 33) on padded pitches, the
    ring kernel also on ldc = ldres = N + 3 with a bf16 residual: against float64 and against tile 22 on the same buffers."""
    _lib.require_gpu()
    lib = _lib.lib()
    p = gc.nt_problem(row, "bf16")
    d = _dev(p)
    knobs = [(0, 256), (1, 256), (1, 128)] if row["tile"] == 88 else [(-1, -1)]
    failures = []
    try:
        lib.sq_dbg_set(0, 22)
        base = _linear(p, d)
        e22, t22 = gc.judge(base, p.idx, p.ref)
        print(f"GEMM_CONTRACT {row['id']} bf16 tile 22: err {e22:.2e} (tol {p.tol:.0e}), {t22} sentinel elements changed")
        if t22 or not e22 < p.tol:
            failures.append((22, e22, t22))
        for sched, bn in knobs:
            lib.sq_dbg_set(10, sched)
            lib.sq_dbg_set(13, bn)
            lib.sq_dbg_set(0, row["tile"])
            flat = _linear(p, d)
            err, touched = gc.judge(flat, p.idx, p.ref)
            vs22 = gc.rel_err(flat[p.idx].float().numpy(), base[p.idx].float().numpy())
            same = bool(torch.equal(_bits(flat), _bits(base)))
            print(f"GEMM_CONTRACT {row['id']} bf16 tile {row['tile']} sched {sched} width {bn}: err {err:.2e} (tol {p.tol:.0e}), "
                  f"{touched} sentinel elements changed, vs tile 22 {vs22:.2e}, bit-equal to tile 22: {same}")
            _note(row["family"], "bf16", err, p.tol)
            if touched or not err < p.tol or not vs22 < p.tol:
                failures.append((row["tile"], sched, bn, err, touched, vs22))
    finally:
        lib.sq_dbg_set(0, 0)
        lib.sq_dbg_set(10, -1)
        lib.sq_dbg_set(13, -1)
    _check_all(failures)


# ---- weight gradients ----
def _tn_dev(p, dtype):
    return p.dY_buf.to("cuda", TORCH[dtype]), p.X_buf.to("cuda", TORCH[dtype])


def _tn_outputs(p):
    assert (p.NO - 1) * p.lddw + p.NI <= p.dw_len and gc.DB_GUARD + p.NO <= p.db_len
    return gc.sentinel(p.dw_len, "f32").cuda(), gc.sentinel(p.db_len, "f32").cuda()


def _tn_judge(p, dw, db, with_db):
    e_dw, t_dw = gc.judge(dw.cpu(), p.idx, p.ref_dw)
    if with_db:
        e_db, t_db = gc.judge(db.cpu(), p.db_idx, p.ref_db)
    else:                                               # no bias gradient asked for: the whole buffer is guard
        e_db, t_db = 0.0, int((_bits(db.cpu()) != gc.SENT32).sum())
    return e_dw, e_db, t_dw + t_db


@pytest.mark.parametrize("row", gc.TN_CASES, ids=lambda r: r["id"])
def test_tn_weight_grad_strides_tiny_extents_and_empty_slices(row, ws):
    """dW and dbias for n_out from 1 (HE2RNA's layers=[1]) to 129, token counts around the 32 / 64-row steps, padded lddy / ldx /
    lddw (lddw = NI + 1: scalar epilogue), with and without dbias; without a workspace, with one, and with sq_dbg_set(4, s)
    chosen so that the last token slice is empty.  One row holds NaN in dY's columns [n_out, round_up(n_out, 8))."""
    _lib.require_gpu()
    lib = _lib.lib()
    p = gc.tn_problem(row)
    failures = []
    for dtype in ("f32", "bf16"):
        dY, X = _tn_dev(p, dtype)
        forced = gc.tn_empty_slice_split(dtype, p.T)
        for with_db in (True, False):
            for mode, split, ws_bytes in (("no workspace", 0, 0), ("workspace", 0, gc.WS64), (f"{forced} forced slices", forced, gc.WS64)):
                dw, db = _tn_outputs(p)
                lib.sq_dbg_set(4, split)
                try:
                    _lib.check(lib.sq_linear_weight_grad(CODE[dtype], _lib.ptr(dY), p.lddy, _lib.ptr(X), p.ldx, _lib.ptr(dw), p.lddw,
                                                         VP(db.data_ptr() + 4 * gc.DB_GUARD) if with_db else None, p.NO, p.NI, p.T,
                                                         _lib.ptr(ws) if ws_bytes else None, ws_bytes, _lib.stream_ptr()))
                    torch.cuda.synchronize()
                finally:
                    lib.sq_dbg_set(4, 0)
                e_dw, e_db, touched = _tn_judge(p, dw, db, with_db)
                print(f"GEMM_CONTRACT {row['id']} {dtype} dbias {int(with_db)} {mode}: dW err {e_dw:.2e} dbias err {e_db:.2e} (tol {p.tol:.0e}), "
                      f"{touched} sentinel elements changed")
                _note("tn", dtype, max(e_dw, e_db), p.tol)
                if touched or not e_dw < p.tol or not e_db < p.tol:
                    failures.append((dtype, with_db, mode, e_dw, e_db, touched))
    _check_all(failures)


@pytest.mark.parametrize("row", gc.GROUP_CASES, ids=lambda r: r["id"])
def test_tn_group_entry_with_padded_leading_dimensions(row):
    """One to four members, all three leading dimensions padded, a ring shape (taken by the ring form from two members on) and a
    shape the ring form does not take, ring on and off, with and without dbias."""
    _lib.require_gpu()
    lib = _lib.lib()
    n = row["members"]
    ps = [gc.tn_problem(row, m) for m in range(n)]
    arr = lambda ptrs: (VP * n)(*ptrs)
    failures = []
    for dtype in row["dtypes"]:
        ops = [_tn_dev(p, dtype) for p in ps]
        for ring in (1, 0):
            for with_db in (True, False):
                outs = [_tn_outputs(p) for p in ps]
                lib.sq_dbg_set(15, ring)
                try:
                    _lib.check(lib.sq_linear_weight_grad_group(CODE[dtype], n, arr([o[0].data_ptr() for o in ops]), arr([o[1].data_ptr() for o in ops]),
                                                               arr([o[0].data_ptr() for o in outs]),
                                                               arr([o[1].data_ptr() + 4 * gc.DB_GUARD for o in outs]) if with_db else None,
                                                               row["lddy"], row["ldx"], row["lddw"], row["NO"], row["NI"], row["T"], _lib.stream_ptr()))
                    torch.cuda.synchronize()
                finally:
                    lib.sq_dbg_set(15, -1)
                for m, (p, (dw, db)) in enumerate(zip(ps, outs)):
                    e_dw, e_db, touched = _tn_judge(p, dw, db, with_db)
                    print(f"GEMM_CONTRACT {row['id']} {dtype} member {m} ring {ring} dbias {int(with_db)}: dW err {e_dw:.2e} dbias err {e_db:.2e} "
                          f"(tol {p.tol:.0e}), {touched} sentinel elements changed")
                    _note("group", dtype, max(e_dw, e_db), p.tol)
                    if touched or not e_dw < p.tol or not e_db < p.tol:
                        failures.append((dtype, m, ring, with_db, e_dw, e_db, touched))
    _check_all(failures)


def test_worst_errors_of_this_run():
    """Not a check of its own: prints the worst observed error per family and dtype of the tests above, and the file's wall time."""
    _lib.require_gpu()
    for (family, dtype, tol), err in sorted(WORST.items()):
        print(f"GEMM_CONTRACT_WORST {family} {dtype} operands, rows held to {tol:.0e}: {err:.2e}")
    print(f"GEMM_CONTRACT_WALL {time.time() - T0:.1f} s since this file was imported")
