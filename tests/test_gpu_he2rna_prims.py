"""The HE2RNA device primitives alone through the C ABI against the references of tests/he2rna_prim_cases.py (float64 autograd for
the top-k family, torch on the CPU for the tile mask, a numpy restatement of Philox4x32-10 for dropout): sq_he2rna_topk_mean,
sq_he2rna_topk_mean_bwd, sq_he2rna_window_topk_mean, sq_he2rna_loss_head, sq_he2rna_tile_mask, sq_he2rna_dropout and
sq_he2rna_dropout_gate.  tests/test_he2rna_prims_host.py shows on the CPU where the bounds come from, that a restatement of the
kernels' arithmetic meets them on every row and that mutated rank, mask, count and tie rules break them.

Every output table sits in a sentinel-filled allocation; what lies outside the entry's contract (columns at or beyond the width,
the floats in front of an offset base pointer, the guard behind the table) must keep its bits.  Every case prints
`HE2RNA_PRIM <id> ...` with its worst figure as a ratio to the bound before it asserts; the last test prints the worst per entry
(profiles/he2rna_prim_errors.txt is that output).

One premise is narrower than "NaN exactly where the reference is NaN": the loss head makes its own grad_out = grad_scale * (pred -
target), so a NaN prediction (0/0) turns its whole gradient column into NaN (0 * NaN), as it does in sq_mse_loss_grad +
sq_he2rna_topk_mean_bwd, where autograd with a NaN grad_out keeps exact zeros at the ranks no k reaches.  Those columns are held to
the bit-equality with the three entries, every other column to float64; sq_he2rna_topk_mean_bwd itself gets a finite grad_out and
is held to the reference's NaN pattern exactly.

Measured on an MI355X, worst ratio to the bound over all rows (profiles/he2rna_prim_errors.txt keeps every row): prediction 0.41
(topk_mean, loss head) and 0.35 (window), gradient 0.50, loss 0.43; tile mask, dropout and gate equal their references in every
bit, the smallest denormal included.  No bound had to be widened and no kernel had to change."""
import numpy as np
import pytest
import torch

import he2rna_prim_cases as pc
from sequoia_pub_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _table(t, off=0):
    """A CPU float32 tensor -> (flat device buffer of SENTINEL with the tensor `off` floats in, GUARD floats behind it; the tensor's
    view into it, whose address is the base pointer the entry gets)."""
    n = t.numel()
    flat = torch.full((off + n + GUARD,), pc.SENTINEL)
    flat[off:off + n] = t.reshape(-1)
    flat = flat.to(DEV)
    return flat, flat[off:off + n].view(t.shape)


def _blank(shape, off=0):
    return _table(torch.full(shape, pc.SENTINEL), off)


def _outside_untouched(flat, off, n):
    return bool((flat[:off] == pc.SENTINEL).all()) and bool((flat[off + n:] == pc.SENTINEL).all())


def _same_bits(a, b):
    """Bit-equal floats, NaN at the same positions (a NaN's payload is not part of any contract here)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    nan = torch.isnan(a)
    return torch.equal(torch.isnan(b), nan) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))


def _ks(ks):
    return np.asarray(ks, dtype=np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# top-k mean, its gradient and the loss head
# ----------------------------------------------------------------------------------------------------------------------
def _topk_mean(scores, ld, mask, ks, scale, B, N, G):
    flat, out = _blank((B, G))
    _lib.call("sq_he2rna_topk_mean", DEV, scores, ld, mask, _ks(ks), len(ks), scale, out, B, N, G)
    return flat, out


def _topk_bwd(scores, ld, mask, ks, scale, gout, B, N, G, off=0):
    flat, grad = _blank((B, max(N, 1), ld), off)         # a refused N = 0 still gets a table with an address
    _lib.call("sq_he2rna_topk_mean_bwd", DEV, scores, ld, mask, _ks(ks), len(ks), scale, gout, grad, ld, B, N, G)
    return flat, grad


def _loss_head(scores, ld, mask, ks, scale, target, gscale, B, N, G, off=0):
    pflat, pred = _blank((B, G))
    gflat, grad = _blank((B, max(N, 1), ld), off)
    loss =torch.full((1,), pc.SENTINEL, device=DEV)
    need = _lib.lib().sq_he2rna_loss_head_workspace_bytes(B, G)
    _lib.call("sq_he2rna_loss_head", DEV, scores, ld, mask, _ks(ks), len(ks), scale, target, gscale, pred, loss, grad, ld, B, N, G,
              workspace=need)
    return pflat, pred, loss, gflat, grad


def _check_topk_row(rid):
    """One row through sq_he2rna_topk_mean, sq_he2rna_topk_mean_bwd and sq_he2rna_loss_head -> list of complaints."""
    r, q = pc.TOPK_BY_ID[rid], pc.topk_inputs(rid)
    B, N, G, ld, ks, scale, off = r["B"], r["N"], r["G"], r["ld"], r["ks"], r["scale"], r["off"]
    ref = pc.topk_reference(rid)
    _, scores = _table(q["scores"], off)
    mask, gout, target = q["mask"].to(DEV), q["grad_out"].to(DEV), q["target"].to(DEV)
    assert scores.data_ptr() % 16 == 4 * (off % 4)
    bad = []
    # forward and backward entries against float64
    pflat, pred = _topk_mean(scores, ld, mask, ks, scale, B, N, G)
    gflat, grad = _topk_bwd(scores, ld, mask, ks, scale, gout, B, N, G, off)
    wp, bp = pc.check_pred(pred.cpu(), ref)
    wg, bg = pc.check_grad(grad[:, :, :G].cpu(), ref["grad"])
    bad += [f"topk_mean: {b}" for b in bp] + [f"topk_mean_bwd: {b}" for b in bg]
    if not (_outside_untouched(pflat, 0, B * G) and _outside_untouched(gflat, off, B * N * ld) and bool((grad[:, :, G:] == pc.SENTINEL).all())):
        bad.append("topk_mean / _bwd wrote outside [:, :G] of their tables")
    # the loss head: bit-equal to the entries above, and against float64 on its own
    gscale = 2.0 / (B * G)
    lpflat, lpred, loss, lgflat, lgrad = _loss_head(scores, ld, mask, ks, scale, target, gscale, B, N, G, off)
    wlp, blp = pc.check_pred(lpred.cpu(), ref)
    go = (np.float32(gscale) * (lpred.cpu().numpy() - q["target"].numpy())).astype(np.float32)      # go = grad_scale * fl32(p - t)
    # a NaN prediction makes its whole gradient column NaN in the kernels (0 * NaN), which no training step can use: those columns
    # are held to the bit-equality with the three entries below, the finite ones to float64
    fin = torch.from_numpy(np.isfinite(go))[:, None, :].expand(B, N, G)
    lref = pc.topk_ref(q["scores"][:, :, :G], q["mask"], ks, scale, torch.from_numpy(np.where(np.isfinite(go), go, np.float32(0))))
    wlg, blg = pc.check_grad(torch.where(fin, lgrad[:, :, :G].cpu().double(), lref["grad"]), lref["grad"])
    bad += [f"loss_head pred: {b}" for b in blp] + [f"loss_head grad: {b}" for b in blg]
    want_loss, got_loss = pc.loss_reference(lpred.cpu(), q["target"]), float(loss)
    wl = 0.0
    if np.isnan(want_loss):
        if not np.isnan(got_loss):
            bad.append(f"loss_head loss {got_loss} where the prediction holds NaN")
    else:
        wl = abs(got_loss - want_loss) / (pc.LOSS_RTOL * abs(want_loss))
        if not wl <= 1.0:
            bad.append(f"loss_head loss {got_loss!r} against {want_loss!r}: {wl:.3e} of the bound")
    if not _same_bits(lpred, pred):
        bad.append("loss_head pred is not bit-equal to sq_he2rna_topk_mean")
    _, mgout = _blank((B, G))
    mloss = torch.empty(1, device=DEV)
    _mse(pred, target, B * G, gscale, mgout, mloss)
    _, tgrad = _topk_bwd(scores, ld, mask, ks, scale, mgout, B, N, G, off)
    if not _same_bits(lgrad[:, :, :G], tgrad[:, :, :G]):
        bad.append("loss_head grad_scores is not bit-equal to sq_mse_loss_grad + sq_he2rna_topk_mean_bwd")
    if not (_outside_untouched(lpflat, 0, B * G) and _outside_untouched(lgflat, off, B * N * ld) and bool((lgrad[:, :, G:] == pc.SENTINEL).all())):
        bad.append("loss_head wrote outside [:, :G] of its tables")
    print(f"HE2RNA_PRIM {rid} B{B} ks {r['ks_kind'] or ks} {r['values']}/{r['mask']} ld {ld} off {off}: topk_mean {wp:.3f}, bwd {wg:.3f}, "
          f"loss_head pred {wlp:.3f} grad {wlg:.3f} loss {wl:.3f} of the bound; {bad if bad else 'ok'}")
    for key, v in (("sq_he2rna_topk_mean pred", wp), ("sq_he2rna_topk_mean_bwd grad", wg), ("sq_he2rna_loss_head pred", wlp),
                   ("sq_he2rna_loss_head grad", wlg), ("sq_he2rna_loss_head loss", wl)):
        _note(key, v)
    return bad


def _mse(pred, target, n, gscale, gout, loss):
    scratch = torch.empty(_lib.lib().sq_train_scratch_bytes(n), dtype=torch.uint8, device=DEV)
    _lib.call("sq_mse_loss_grad", DEV, pred, target, n, gscale, gout, loss, scratch)


@pytest.mark.parametrize("N", pc.NS)
def test_topk_entries_and_loss_head_against_float64(N):
    """Every row of the table with this many tiles: prediction and gradient within the derived bounds, NaN and exact zeros where the
    reference has them, the loss head bit-equal to the three entries, nothing written outside [:, :G]."""
    _lib.require_gpu()
    rows = [r["id"] for r in pc.TOPK_ROWS if r["N"] == N]
    assert rows
    bad = {rid: b for rid in rows for b in [_check_topk_row(rid)] if b}
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# sliding windows
# ----------------------------------------------------------------------------------------------------------------------
def _window(scores, ld, mask, idx, ks, scale, nw, N, G):
    flat, out = _blank((nw, G))
    _lib.call("sq_he2rna_window_topk_mean", DEV, scores, ld, mask, pc.GATHER_ROWS, idx, _ks(ks), len(ks), scale, out, nw, N, G)
    return flat, out


@pytest.mark.parametrize("N", pc.WIN_NS)
def test_window_topk_mean_against_float64_and_the_materialised_batch(N):
    _lib.require_gpu()
    bad = {}
    for r in (r for r in pc.WIN_ROWS if r["N"] == N):
        q, ref = pc.win_inputs(r["id"]), pc.win_reference(r["id"])
        G, ld, nw, ks, scale = r["G"], r["ld"], r["n_windows"], r["ks"], r["scale"]
        flat, out = _window(q["scores"].to(DEV), ld, q["mask"].to(DEV), q["idx"].to(DEV), ks, scale, nw, N, G)
        worst, b = pc.check_pred(out.cpu(), ref)
        s, m = pc.win_batch(r["id"])
        _, dense = _topk_mean(s.to(DEV), G, m.to(DEV), ks, scale, nw, N, G)
        if not _same_bits(out, dense):
            b.append("not bit-equal to sq_he2rna_topk_mean on the materialised batch")
        if not _outside_untouched(flat, 0, nw * G):
            b.append("wrote behind out[n_windows, G]")
        print(f"HE2RNA_PRIM {r['id']} windows {nw} ks {r['ks_kind']} ld {ld}: window_topk_mean {worst:.3f} of the bound; {b if b else 'ok'}")
        _note("sq_he2rna_window_topk_mean pred", worst)
        if b:
            bad[r["id"]] = b
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_topk_entries_refuse_by_message_and_compute_the_same_bits_afterwards():
    _lib.require_gpu()
    rid = "n7-g129"
    r, q = pc.TOPK_BY_ID[rid], pc.topk_inputs(rid)
    B, N, G, ld = r["B"], r["N"], r["G"], r["ld"]
    scores, mask, gout, target = q["scores"].to(DEV), q["mask"].to(DEV), q["grad_out"].to(DEV), q["target"].to(DEV)
    wq = pc.win_inputs("w-n7-g129")
    wr = pc.WIN_BY_ID["w-n7-g129"]
    ws, wm, wi = wq["scores"].to(DEV), wq["mask"].to(DEV), wq["idx"].to(DEV)

    entries = {
        "topk_mean": lambda N=N, ks=[2], ld=ld: _topk_mean(scores, ld, mask, ks, 1.0, B, N, G)[1],
        "topk_mean_bwd": lambda N=N, ks=[2], ld=ld: _topk_bwd(scores, ld, mask, ks, 1.0, gout, B, N, G)[1],
        "window_topk_mean": lambda N=N, ks=[2], ld=wr["ld"]: _window(ws, ld, wm, wi, ks, 1.0, wr["n_windows"], N, wr["G"])[1],
        "loss_head": lambda N=N, ks=[2], ld=ld: torch.cat([t.reshape(-1) for t in _loss_head(scores, ld, mask, ks, 1.0, target, 0.5, B, N, G)[1:5:3]]),
    }
    refusals = [(dict(N=0), "0 tiles per"), (dict(N=129), "129 tiles per"), (dict(ks=[0]), "k=0 out of range"),
                (dict(ks=[N + 1]), f"k={N + 1} out of range"), (dict(ks=[]), "0 values of k"), (dict(ks=[1] * 17), "17 values of k"),
                (dict(ld=G - 1), "bad arguments")]
    for name, fn in entries.items():
        before = fn().clone()
        for kwargs, message in refusals:
            if name == "window_topk_mean" and "ld" in kwargs:
                kwargs = dict(ld=wr["G"] - 1)
            with pytest.raises(_lib.SequoiaHipArgError, match=message):
                fn(**kwargs)
            assert _same_bits(fn(), before), (name, kwargs)
        print(f"HE2RNA_PRIM refusals sq_he2rna_{name}: {len(refusals)} refused by message, the same bits afterwards")


# ----------------------------------------------------------------------------------------------------------------------
# tile mask
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", pc.MASK_CS)
def test_tile_mask_equals_torch_on_every_special_row(C):
    """All negative, all +0.0, all -0.0, the only positive value in the last channel (and at channel 64 of 65), the smallest
    denormal among zeros, +inf and all -inf; 1, 3, 4, 5 and 1027 rows (four rows to a block); a sentinel behind mask[rows]."""
    _lib.require_gpu()
    bad = {}
    for rows in pc.MASK_ROWS:
        x, want = pc.tile_mask_case(rows, C)
        flat, mask = _blank((rows,))
        _lib.call("sq_he2rna_tile_mask", DEV, torch.from_numpy(x).to(DEV), rows, C, mask)
        got = mask.cpu().numpy()
        wrong = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
        sp = pc.tile_mask_specials(rows, C)
        print(f"HE2RNA_PRIM tile_mask rows {rows} C {C}: {wrong.size} of {rows} rows differ" +
              (f", first row {int(wrong[0])} ({sp.get(int(wrong[0]), 'ordinary')}): got {got[wrong[0]]}, want {want[wrong[0]]}" if wrong.size else ""))
        _note("sq_he2rna_tile_mask rows unequal", wrong.size)
        if wrong.size or not _outside_untouched(flat, 0, rows):
            bad[rows] = ([(int(i), sp.get(int(i), "ordinary")) for i in wrong[:8]], _outside_untouched(flat, 0, rows))
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# dropout and its gate
# ----------------------------------------------------------------------------------------------------------------------
def _bits(flat):
    return flat.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("width", pc.WIDTHS)
def test_dropout_equals_the_philox_reference_bit_for_bit(width):
    """Every byte of the allocation: kept elements scaled, dropped ones +0.0, columns at or beyond the width, the floats in front of
    an offset base pointer and the guard behind the table unchanged."""
    _lib.require_gpu()
    bad = {}
    for c in (c for c in pc.DROPOUT_CASES if c["width"] == width):
        x = pc.dropout_input(c)
        flat, _ = pc.embed(x, c["ld"], c["off"])
        want, _ = pc.embed(pc.dropout_reference(x, c["p"], c["seed"], c["step"], c["layer"]), c["ld"], c["off"])
        dev = torch.from_numpy(flat).to(DEV)
        _lib.call("sq_he2rna_dropout", DEV, dev[c["off"]:], c["ld"], c["rows"], width, c["p"], c["seed"], c["step"], c["layer"])
        wrong = np.flatnonzero(_bits(dev) != want.view(np.int32))
        print(f"HE2RNA_PRIM {c['id']} ld {c['ld']} p {c['p']!r} seed {c['seed']:#x} layer {c['layer']} step {c['step']}: {wrong.size} of {flat.size} floats differ")
        _note("sq_he2rna_dropout floats unequal", wrong.size)
        if wrong.size:
            bad[c["id"]] = (wrong.size, int(wrong[0]))
    assert not bad, bad


def test_dropout_refuses_a_step_of_2_to_the_32_and_a_negative_layer():
    _lib.require_gpu()
    buf = torch.rand(7, 16, device=DEV)
    before = buf.clone()
    for step, layer in ((2 ** 32, 0), (0, -1), (-1, 0)):
        with pytest.raises(_lib.SequoiaHipArgError, match="step index"):
            _lib.call("sq_he2rna_dropout", DEV, buf, 16, 7, 13, 0.5, 1, step, layer)
    with pytest.raises(_lib.SequoiaHipArgError, match="p = 1 must be in"):
        _lib.call("sq_he2rna_dropout_gate", DEV, buf, 16, before, 16, 7, 13, 1.0)
    assert torch.equal(buf, before)


@pytest.mark.parametrize("width", pc.WIDTHS)
def test_dropout_gate_selects_and_scales_bit_for_bit(width):
    """act > 0 ? fl32(grad * inv_keep) : +0.0 with act holding +0.0, -0.0, the smallest denormal, negative values and NaN, and inf and
    NaN gradients at dropped positions; act and everything outside the width keep their bits; p = 0 leaves kept gradients as
    they are.  Both tables aligned (16-byte accesses), and every mix in which one of them forces the scalar path."""
    _lib.require_gpu()
    bad = {}
    for c in (c for c in pc.GATE_CASES if c["width"] == width):
        grad, act = pc.gate_inputs(c)
        gflat, _ = pc.embed(grad, c["ld_grad"], c["off_grad"])
        aflat, _ = pc.embed(act, c["ld_act"], c["off_act"])
        want, _ = pc.embed(pc.gate_reference(grad, act, c["p"]), c["ld_grad"], c["off_grad"])
        gdev, adev = torch.from_numpy(gflat).to(DEV), torch.from_numpy(aflat).to(DEV)
        _lib.call("sq_he2rna_dropout_gate", DEV, gdev[c["off_grad"]:], c["ld_grad"], adev[c["off_act"]:], c["ld_act"], c["rows"], width, c["p"])
        wrong = np.flatnonzero(_bits(gdev) != want.view(np.int32))
        act_changed = int(np.count_nonzero(_bits(adev) != aflat.view(np.int32)))
        print(f"HE2RNA_PRIM {c['id']} ld {c['ld_grad']}/{c['ld_act']} p {c['p']}: {wrong.size} of {gflat.size} gradient floats differ, {act_changed} of act changed")
        _note("sq_he2rna_dropout_gate floats unequal", wrong.size + act_changed)
        if wrong.size or act_changed:
            i = int(wrong[0]) if wrong.size else -1
            bad[c["id"]] = (wrong.size, act_changed, i, None if i < 0 else (float(_bits(gdev).view(np.float32)[i]), float(want[i])))
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# the record
# ----------------------------------------------------------------------------------------------------------------------
def test_zz_print_the_worst_figure_per_entry():
    """Runs last in the module: the table profiles/he2rna_prim_errors.txt keeps (ratios to the bound; counts for the bit-equal entries)."""
    _lib.require_gpu()
    print("\nHE2RNA_PRIM worst figure per entry (ratio to the bound, or number of unequal elements)")
    for key in sorted(WORST):
        print(f"HE2RNA_PRIM_WORST {key:45s} {WORST[key]:.3f}")
    assert all(v <= 1.0 for k, v in WORST.items() if "unequal" not in k) and all(v == 0 for k, v in WORST.items() if "unequal" in k)
