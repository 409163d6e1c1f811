"""CPU checks of tests/he2rna_prim_cases.py: the tables cover what they name, the Philox restatement gives the three known
answers, the float64 top-k reference agrees with oracle/he2rna_oracle.py where torch.topk's tie order cannot matter, a CPU
emulation of he2rna_topk_kernel's arithmetic stays within every bound on every row (so the bounds are met by a correct kernel),
and every mutated reference breaks a bound on a named row (so the bounds have teeth).  Prints `HE2RNA_PRIM_HOST ...` lines with the
measured figures."""
import os
import re

import numpy as np
import pytest
import torch

import he2rna_prim_cases as pc
from oracle import he2rna_oracle as ho


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def test_topk_table_covers_what_it_names():
    rows = pc.TOPK_ROWS
    assert len({r["id"] for r in rows}) == len(rows)
    pairs = {(r["N"], r["G"]) for r in rows}
    assert {r["N"] for r in rows} == set(pc.NS) and {r["G"] for r in rows} == set(pc.GS) and {r["B"] for r in rows} == {1, 3}
    assert all((N, G) in pairs for N in pc.NS for G in (1, 129, 257)) and all((N, G) in pairs for G in pc.GS for N in (9, 128))
    assert {r["ks_kind"] for r in rows} >= set(pc.KS_KINDS) and {r["values"] for r in rows} == set(pc.VALUE_KINDS)
    assert {r["mask"] for r in rows} == set(pc.MASK_KINDS) and {r["scale_kind"] for r in rows} == set(pc.SCALES)
    assert {r["ld_kind"] for r in rows} == set(pc.LD_KINDS) and {r["off"] for r in rows} == {0, 1}
    for r in rows:
        assert 1 <= r["N"] <= pc.MAX_N and 1 <= len(r["ks"]) <= pc.MAX_KS and all(1 <= k <= r["N"] for k in r["ks"]) and r["ld"] >= r["G"]
    assert len(pc.SIXTEEN) == pc.MAX_KS and len(set(pc.SIXTEEN)) == 16
    # the three ranking loops of the blocked kernels (blocks of 8) meet at these N; 256- and 128-wide gene blocks at these G
    assert {8, 9, 16, 17, 127} <= set(pc.NS) and {127, 128, 129, 255, 256, 257} <= set(pc.GS)
    # quantised rows do have live ties inside the top max(ks) of some column, Gaussian ones have none among live scores
    for r in rows:
        q = pc.topk_inputs(r["id"])
        s = (q["scores"][:, :, :r["G"]] * q["mask"][:, :, None])
        assert bool((q["scores"][:, :, r["G"]:] == pc.POISON).all())
        if r["values"] == "quant" and r["N"] >= 16:
            t = torch.sort(s, dim=1, descending=True).values[:, :max(r["ks"])]
            assert bool((t[:, 1:] == t[:, :-1]).any()), r["id"]
        if pc.is_tie_free(r["id"]):
            live = torch.where(q["mask"][:, :, None] > 0, s, torch.arange(r["N"])[None, :, None] + 100.0)
            t = torch.sort(live, dim=1).values
            assert bool((t[:, 1:] != t[:, :-1]).all()) and bool((q["mask"][:, 0] == 1).all()), r["id"]
        if r["values"] == "neg":
            assert bool((s <= 0).all()) and bool((q["mask"] == 0).any())
        if r["values"] == "zeros":
            live0 = (s == 0) & (q["mask"][:, :, None] > 0)
            assert bool((live0 & torch.signbit(s)).any()) and bool((live0 & ~torch.signbit(s)).any())


def test_window_table_covers_what_it_names():
    rows = pc.WIN_ROWS
    assert {(r["N"], r["G"]) for r in rows} == {(N, G) for N in pc.WIN_NS for G in pc.WIN_GS}
    for N in pc.WIN_NS:
        assert {r["n_windows"] for r in rows if r["N"] == N} == {1, 37}
    for G in pc.WIN_GS:
        assert {r["n_windows"] for r in rows if r["G"] == G} == {1, 37}
    assert {r["ks_kind"] for r in rows} == set(pc.KS_KINDS)
    seen_pad, seen_max = 0, False
    for r in rows:
        q = pc.win_inputs(r["id"])
        idx = q["idx"]
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (r["n_windows"], r["N"])
        if r["N"] >= 7 and r["n_windows"] == 37:
            assert bool((idx == -1).any()) and bool((idx >= pc.GATHER_ROWS).any())
        if r["N"] >= 8:
            live = (idx >= 0) & (idx < pc.GATHER_ROWS)
            assert bool((idx[:, 5] == idx[:, 2])[torch.arange(len(idx)) != pc.WIN_PAD_WINDOW].all())      # one table row twice in a window
            assert r["n_windows"] == 1 or bool(live[:, 2].any())
        if r["n_windows"] > pc.WIN_PAD_WINDOW:
            _, m = pc.win_batch(r["id"])
            assert float(m[pc.WIN_PAD_WINDOW, :max(r["ks"])].sum()) == 0
            assert bool(torch.isnan(pc.win_reference(r["id"])["pred"][pc.WIN_PAD_WINDOW]).all())
            seen_pad += 1
        seen_max = seen_max or bool((idx == 2 ** 31 - 1).any())
    assert seen_pad >= 5 and seen_max


def test_elementwise_tables_cover_what_they_name():
    d = pc.DROPOUT_CASES
    assert {c["width"] for c in d} == set(pc.WIDTHS) and {c["rows"] for c in d} == set(pc.ELEM_ROWS) and {c["off"] for c in d} == {0, 1}
    assert {(c["p"], c["seed"], c["layer"], c["step"]) for c in d} == {(p, s, la, st) for p in pc.DROP_PS for s in pc.DROP_SEEDS
                                                                        for la in pc.DROP_LAYERS for st in pc.DROP_STEPS}
    for w in pc.WIDTHS:
        mine = [c for c in d if c["width"] == w]
        assert {pc.takes_vector_path(c["ld"], c["off"]) for c in mine} == {True, False}
        assert any(c["ld"] % 4 != 0 for c in mine) and any(c["ld"] == w for c in mine) and all(c["ld"] >= w for c in mine)
    assert any(c["rows"] * -(-c["width"] // 4) > 256 for c in d) and any(c["rows"] * -(-c["width"] // 4) < 256 for c in d)
    g = pc.GATE_CASES
    assert {c["width"] for c in g} == set(pc.WIDTHS) and {c["p"] for c in g} == set(pc.GATE_PS)
    assert all(c["ld_grad"] != c["ld_act"] for c in g)
    vec = {(pc.takes_vector_path(c["ld_grad"], c["off_grad"]), pc.takes_vector_path(c["ld_act"], c["off_act"])) for c in g}
    assert {(True, True), (True, False), (False, True)} <= vec           # 16-byte accesses, and either table alone forcing the scalar path
    for c in g[:12]:
        grad, act = pc.gate_inputs(c)
        want = pc.gate_reference(grad, act, c["p"])
        with np.errstate(invalid="ignore"):
            dropped = ~(act > 0)
        assert not np.isnan(want[dropped]).any() and (want[dropped].view(np.int32) == 0).all()
        if c["p"] == 0.0:
            assert (want[~dropped].view(np.int32) == grad[~dropped].view(np.int32)).all()
    grad, act = pc.gate_inputs(pc.GATE_CASES[-1])
    assert np.isnan(act).any() and (act == pc.DENORM_MIN).any() and np.signbit(act[act == 0]).any() and (act < 0).any()
    assert np.isinf(grad).any() and np.isnan(grad).any()
    assert pc.gate_reference(np.float32([3.0]), np.float32([1e-45]), 0.5)[0] == 6.0


def test_tile_mask_cases_hold_every_special_row_at_every_width():
    for C in pc.MASK_CS:
        kinds = set()
        for rows in pc.MASK_ROWS:
            sp = pc.tile_mask_specials(rows, C)
            kinds |= set(sp.values())
            x, want = pc.tile_mask_case(rows, C)
            assert x.shape == (rows, C) and not np.isnan(x).any()
            for r, kind in sp.items():
                lit = kind in ("positive_last", "positive_at_64", "denormal", "pos_inf")
                assert want[r] == (1.0 if lit else 0.0), (rows, C, r, kind)
        assert kinds == set(pc.MASK_SPECIALS)
        x, want = pc.tile_mask_case(1027, C)
        assert 0 < want.sum() < 1027
    assert pc.DENORM_MIN.view(np.int32) == 1


# ----------------------------------------------------------------------------------------------------------------------
# Philox and dropout
# ----------------------------------------------------------------------------------------------------------------------
def test_philox_restatement_gives_the_three_known_answers():
    for counter, key, want in pc.PHILOX_KNOWN_ANSWERS:
        got = tuple(int(w) for w in pc.philox4x32_10(counter, key))
        print("HE2RNA_PRIM_HOST philox", " ".join(f"{w:08x}" for w in got))
        assert got == want
    # arrays go through word for word
    got = pc.philox4x32_10((np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344])),
                           (np.array([0, 0xa4093822]), np.array([0, 0x299f31d0])))
    assert [int(w[0]) for w in got] == list(pc.PHILOX_KNOWN_ANSWERS[0][2]) and [int(w[1]) for w in got] == list(pc.PHILOX_KNOWN_ANSWERS[2][2])


def test_dropout_reference_keep_rates_and_teeth():
    c = pc.DROPOUT_BY_ID[pc.DROPOUT_TEETH_CASE]
    assert c["rows"] == 7 and c["width"] == 13
    hi_seed = 0x1234567800000001
    base = pc.dropout_keep(7, 13, 0.5, hi_seed, 0, 0)
    for mutate in ("swap_counter", "low_key"):
        other = pc.dropout_keep(7, 13, 0.5, hi_seed, 0, 0, mutate=mutate)
        print(f"HE2RNA_PRIM_HOST dropout {mutate}: {int((other != base).sum())} of 91 keep flags change")
        assert int((other != base).sum()) >= 20
    assert not np.array_equal(base, pc.dropout_keep(7, 13, 0.5, hi_seed, 1, 0)) and not np.array_equal(base, pc.dropout_keep(7, 13, 0.5, hi_seed, 0, 3))
    assert not np.array_equal(pc.dropout_keep(7, 13, 0.5, -1, 0, 0), pc.dropout_keep(7, 13, 0.5, 0xFFFFFFFF, 0, 0))
    keep = pc.dropout_keep(300, 64, 0.1, 1234, 0, 0)
    assert abs(keep.mean() - 0.9) < 5 * (0.09 / keep.size) ** 0.5
    assert pc.dropout_keep(300, 64, 2.0 ** -24, 1234, 0, 0).mean() > 0.9999 and pc.dropout_keep(300, 64, 1 - 2.0 ** -24, 1234, 0, 0).mean() < 1e-4
    x = pc.dropout_input(c)
    out = pc.dropout_reference(x, 0.5, 1234, 0, 0)
    kept = pc.dropout_keep(7, 13, 0.5, 1234, 0, 0)
    assert (out[kept] == 2 * x[kept]).all() and (out[~kept].view(np.int32) == 0).all()
    assert np.float32(1) / (np.float32(1) - np.float32(1 - 2.0 ** -24)) == np.float32(2.0 ** 24)


# ----------------------------------------------------------------------------------------------------------------------
# top-k reference
# ----------------------------------------------------------------------------------------------------------------------
def test_reference_orders_ties_and_signed_zeros_as_the_header_says():
    v = torch.tensor([0.0, -0.0, 1.0, 0.0, 1.0, -1.0], dtype=torch.float64)
    assert torch.sort(v, descending=True, stable=True).indices.tolist() == [2, 4, 0, 1, 3, 5]
    # the 0/0 pattern: mask [0, 0, 1, 1, 0, 1], ks [2, 4]
    g = torch.Generator().manual_seed(0)
    scores, mask = torch.randn(1, 6, 3, generator=g), torch.tensor([[0.0, 0, 1, 1, 0, 1]])
    ref = pc.topk_ref(scores, mask, [2, 4], 0.5, torch.ones(1, 3))
    assert bool(torch.isnan(ref["pred"]).all())
    s = scores.double() * mask[..., None]
    rank = torch.argsort(torch.sort(s, dim=1, descending=True, stable=True).indices, dim=1)
    assert torch.equal(torch.isnan(ref["grad"]), rank < 2) and bool((rank < 2)[:, [0, 1, 4]].any())
    pred, grad = pc.topk_emulate(scores, mask, [2, 4], 0.5, torch.ones(1, 3))
    assert bool(torch.isnan(pred).all()) and torch.equal(torch.isnan(grad), rank < 2)


def test_reference_equals_the_oracle_on_tie_free_rows():
    rows = [r for r in pc.TOPK_ROWS if pc.is_tie_free(r["id"])]
    assert len(rows) >= 8
    worst = 0.0
    for r in rows:
        q = pc.topk_inputs(r["id"])
        scores, mask, go = q["scores"][:, :, :r["G"]], q["mask"], q["grad_out"].double()

        def oracle(fn):
            leaf = scores.double().clone().requires_grad_(True)
            sd, x, d = pc.oracle_inputs(leaf, mask)
            out = fn(sd, x, d)
            (out * go).sum().backward()
            return out.detach(), leaf.grad

        cases = [([k], 1.0, lambda sd, x, d, k=k: ho.forward_fixed_k(sd, x, k, d)) for k in sorted(set(r["ks"]))]
        cases.append((r["ks"], 1.0 / len(r["ks"]), lambda sd, x, d: ho.forward_eval(sd, x, r["ks"], d)))
        for ks, scale, fn in cases:
            ref = pc.topk_ref(scores, mask, ks, scale, q["grad_out"], round_scale=False)
            out, grad = oracle(fn)
            e = max(float((out - ref["pred"]).abs().max()), float((grad - ref["grad"]).abs().max()))
            worst = max(worst, e)
            assert e <= 1e-12, (r["id"], ks, e)
    print(f"HE2RNA_PRIM_HOST oracle agreement over {len(rows)} tie-free rows: worst |difference| {worst:.2e}")


@pytest.mark.parametrize("rid", [r["id"] for r in pc.TOPK_ROWS])
def test_emulated_kernel_arithmetic_meets_the_bounds(rid):
    r, q = pc.TOPK_BY_ID[rid], pc.topk_inputs(rid)
    ref = pc.topk_reference(rid)
    figs = []
    for fma in (False, True):
        pred, grad = pc.topk_emulate(q["scores"][:, :, :r["G"]], q["mask"], r["ks"], r["scale"], q["grad_out"], fma=fma)
        wp, bad_p = pc.check_pred(pred, ref)
        wg, bad_g = pc.check_grad(grad, ref["grad"])
        figs.append((wp, wg))
        assert not bad_p and not bad_g, (rid, fma, bad_p, bad_g)
    print(f"HE2RNA_PRIM_HOST emulation {rid}: prediction {figs[0][0]:.3f} (fma {figs[1][0]:.3f}) of the bound, gradient {figs[0][1]:.3f}")
    # a slide's prediction is NaN exactly when one of its k reaches only masked positions (0/0)
    empty = torch.stack([q["mask"][:, :k].sum(1) == 0 for k in r["ks"]]).any(0)
    assert torch.equal(torch.isnan(ref["pred"]), empty[:, None].expand(r["B"], r["G"]))
    assert bool(empty.any()) == (rid in pc.NAN_ROWS) and torch.equal(torch.isnan(ref["grad"]).flatten(1).any(1), empty)
    if not bool(empty.any()) and r["values"] != "neg":       # neg: a masked zero can hold every rank below max(ks), a zero gradient is right
        assert float(ref["grad"].abs().max()) > 0


@pytest.mark.parametrize("rid", [r["id"] for r in pc.WIN_ROWS])
def test_emulated_window_arithmetic_meets_the_bounds(rid):
    r = pc.WIN_BY_ID[rid]
    s, m = pc.win_batch(rid)
    ref = pc.win_reference(rid)
    pred, _ = pc.topk_emulate(s, m, r["ks"], r["scale"])
    worst, bad = pc.check_pred(pred, ref)
    print(f"HE2RNA_PRIM_HOST emulation {rid}: prediction {worst:.3f} of the bound")
    assert not bad, (rid, bad)


@pytest.mark.parametrize("mutate", pc.MUTATIONS)
def test_every_mutated_reference_breaks_a_bound_on_its_named_row(mutate):
    rid = pc.TEETH_ROWS[mutate]
    r, q = pc.TOPK_BY_ID[rid], pc.topk_inputs(rid)
    wrong = pc.topk_reference(rid, mutate)
    pred, grad = pc.topk_emulate(q["scores"][:, :, :r["G"]], q["mask"], r["ks"], r["scale"], q["grad_out"])
    wp, bad_p = pc.check_pred(pred, wrong)
    wg, bad_g = pc.check_grad(grad, wrong["grad"])
    print(f"HE2RNA_PRIM_HOST mutation {mutate} on {rid}: prediction {wp:.3e}, gradient {wg:.3e} times the bound")
    assert bad_g, (mutate, rid)
    if mutate != "ties_larger_first":                # the tie order moves no value, only where the gradient goes
        assert bad_p, (mutate, rid)


def test_every_he2rna_entry_that_launches_a_kernel_is_named_by_a_reference_test():
    """The HE2RNA sections of the header against the GPU modules: the primitives by tests/test_gpu_he2rna_prims.py, the two whole passes
    by He2rnaTrainStep, which tests/test_gpu_he2rna_train.py holds to the float64 trajectory of tests/he2rna_train_cases.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "sequoia_hip.h")) as f:
        entries = set(re.findall(r"^(?:int|size_t) (sq_he2rna_\w+)\(", f.read(), flags=re.M))
    sizes_only = {"sq_he2rna_param_layout", "sq_he2rna_loss_head_workspace_bytes", "sq_he2rna_train_workspace_bytes"}
    passes = {"sq_he2rna_train_forward", "sq_he2rna_train_backward"}
    assert sizes_only | passes < entries and len(entries) == 12
    with open(os.path.join(root, "tests", "test_gpu_he2rna_prims.py")) as f:
        prims = f.read()
    for name in entries - sizes_only - passes:
        assert f'"{name}"' in prims, name
    with open(os.path.join(root, "sequoia-pub_amd", "he2rna.py")) as f:
        step = f.read()
    with open(os.path.join(root, "tests", "test_gpu_he2rna_train.py")) as f:
        assert all(f'"{name}"' in step for name in passes) and "He2rnaTrainStep" in f.read()
