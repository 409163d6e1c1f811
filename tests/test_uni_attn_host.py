"""The checker of tests/test_gpu_uni_attn.py on trial, on the CPU (tests/uni_attn_cases.py): it has to accept what a correct
kernel does -- the roundings of the bf16 MFMA core emulated in torch, and plain float32 arithmetic -- and to reject, even at the
loosest (bf16) bound, a core that leaks a zero key, drops the last key, copies the last query row from the one before, swaps two
V rows, swaps the heads or swaps the images, in at least one input family at every T >= 2."""
import pytest
import torch

import uni_attn_cases as ac


def test_token_counts_are_the_admitted_image_sizes_and_the_tile_edges():
    assert ac.PRODUCTION_T == (2, 5, 10, 17, 26, 37, 50, 65, 82, 101, 122, 145, 170, 197, 226)
    assert set(ac.EDGE_T) <= set(ac.ALL_T) and len(ac.ALL_T) == 22 and max(ac.ALL_T) == 256
    assert ac.HEADS & (ac.HEADS - 1) and ac.N_IMG >= 2


@pytest.mark.parametrize("T", ac.ALL_T)
def test_inputs_are_what_the_families_promise(T):
    for fam in ac.FAMILIES:
        d = ac.inputs(fam, T)
        for t in (d["q"], d["k"], d["v"]):
            assert t.shape == (ac.N_IMG, ac.HEADS, T, 64) and torch.equal(t, t.to(torch.bfloat16).double())
        flat = torch.cat([d["k"], d["v"]], -1).reshape(ac.N_IMG * ac.HEADS, -1)
        if not (fam == "readback" and T == 1):                   # one +-1 code of one key may repeat; v = +-1 does
            assert len({tuple(r.tolist()) for r in flat}) == ac.N_IMG * ac.HEADS, "every (image, head) has data of its own"
    b = ac.inputs("bait", T)
    s = 0.125 * (b["q"] @ b["k"].transpose(-2, -1))
    assert float(s.max()) < -10.0 and float(s.min()) > -14.0
    true = ac.attention64(b["q"], b["k"], b["v"])
    leaked = ac.MUTANTS["one zero key leaked"](b["q"], b["k"], b["v"])
    assert float(true.min()) >= 1.0 and float(leaked.max()) <= (2.2e-3 if T <= 226 else 2.5e-3)      # ~ T e^-12 max v
    r = ac.inputs("readback", T)
    o = ac.attention64(r["q"], r["k"], r["v"])
    assert bool(((o.abs() - (r["perm"][..., None] + 1.0)).abs() < 0.1).all())
    assert bool((o[..., 0::2] > 0).all()) and bool((o[..., 1::2] < 0).all())


@pytest.mark.parametrize("T", ac.ALL_T)
def test_checker_accepts_the_roundings_of_a_correct_kernel(T):
    for fam in ac.FAMILIES:
        d = ac.inputs(fam, T)
        ok32, r32 = ac.verdict("fp32", ac.float32_core(d["q"], d["k"], d["v"]), **d)
        okbf, rbf = ac.verdict("bf16", ac.emulate_bf16_core(d["q"], d["k"], d["v"]), **d)
        print(f"T {T:3d} {fam:8s}: float32 uses {r32:.3f} of its bound, the bf16 emulation {rbf:.3f}")
        assert ok32 and okbf, (fam, r32, rbf)
        assert ac.verdict("fp32", ac.attention64(d["q"], d["k"], d["v"]), **d) == (True, 0.0)


@pytest.mark.parametrize("name", list(ac.MUTANTS))
@pytest.mark.parametrize("T", [t for t in ac.ALL_T if t >= 2])
def test_checker_rejects_a_wrong_core_in_some_family(T, name):
    caught = []
    for fam in ac.FAMILIES:
        d = ac.inputs(fam, T)
        ok, ratio = ac.verdict("bf16", ac.MUTANTS[name](d["q"], d["k"], d["v"]), **d)
        if not ok:
            caught.append(fam)
    assert caught, f"{name} at T = {T} passes the bf16 bound in every family"
