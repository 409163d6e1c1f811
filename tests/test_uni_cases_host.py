"""CPU side of the UNI shape sweep (tests/uni_cases.py): is every row a fair test?  The float32 oracle must sit a decade inside
the fp32 bound of the float64 oracle, the bfloat16 CPU oracle inside the bf16 bound, and the bounds must have teeth: an
attention core that leaks a padding key, drops the last key or takes the last query row from the row before has to move the
features by more than three times the fp32 bound at every row of two key tiles or more.  (The bf16 bound of 5e-2 does not see
them -- tests/test_gpu_uni_attn.py holds the bf16 core to its own bound for that reason.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

import uni_cases as uc
from gpu_util import rel_err
from oracle import uni_oracle
from sequoia_pub_amd import _abi, _lib
from sequoia_pub_amd.uni import UniConfig, UniLayout, UniViT

MAX_DEPTH = _abi.CONSTANTS["SQ_UNI_MAX_DEPTH"]
IDS = [c["id"] for c in uc.CASES]
TWO_TILES = [c["id"] for c in uc.CASES if c["T"] > 32]


def test_table_covers_the_admitted_token_range_and_the_branches_it_names():
    ts = {c["T"] for c in uc.CASES}
    assert {2, 17, 37, 65, 101, 145, 226} <= ts and max(ts) == 226
    assert all(c["depth"] >= 2 for c in uc.CASES[:-1]) and uc.CASES[-1]["depth"] == 1
    assert any(c["dim"] == 4096 for c in uc.CASES) and any(c["dim"] == 1024 and c["T"] == 226 for c in uc.CASES)
    assert any(c["dim"] % 128 for c in uc.CASES) and any(c["n"] == 1 for c in uc.CASES)
    assert all(c["branch"] for c in uc.CASES)
    assert uc.BY_ID[uc.AFTER_REFUSAL]["T"] > 32


@pytest.mark.parametrize("cid", IDS)
def test_float32_oracle_is_a_decade_inside_the_fp32_bound(cid):
    c = uc.BY_ID[cid]
    d = rel_err(uc.reference(c, torch.float32), uc.reference(c))
    print(f"{cid}: float32 oracle vs float64 oracle {d:.2e}   [{c['branch']}]")
    assert np.isfinite(uc.reference(c)).all() and uc.reference(c).shape == (c["n"], c["dim"])
    assert d < uc.FLOOR_F32


@pytest.mark.parametrize("cid", IDS)
def test_bfloat16_oracle_is_inside_the_bf16_bound(cid):
    c = uc.BY_ID[cid]
    d = rel_err(uc.reference(c, torch.bfloat16), uc.reference(c))
    print(f"{cid}: bfloat16 oracle vs float64 oracle {d:.2e}")
    assert d < uc.TOL["bf16"]


@pytest.mark.parametrize("name", list(uc.MUTATIONS))
@pytest.mark.parametrize("cid", TWO_TILES)
def test_a_wrong_attention_core_would_show_in_the_fp32_and_f16x3_bounds(monkeypatch, cid, name):
    c = uc.BY_ID[cid]
    monkeypatch.setattr(uni_oracle, "attention", uc.MUTATIONS[name](uni_oracle.attention))
    moved = rel_err(uc.reference_uncached(c, torch.float64), uc.reference(c))
    print(f"{cid}: {name} moves the features by {moved:.2e}")
    assert moved > uc.TEETH


def test_factored_attention_left_the_oracle_bit_equal():
    """forward() with attention() against the same lines written out in place, as they stood before the factoring."""
    c = uc.BY_ID["uni-D192-h3-F200-S160-L2-n2"]
    sd, x = uc.state_dict(c), uni_oracle.transform_patch_u8(uc.patches(c))
    F = torch.nn.functional
    with torch.no_grad():
        got = uni_oracle.forward(sd, x, c["heads"])
        B, D, heads = x.shape[0], c["dim"], c["heads"]
        t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
        t = torch.cat([sd["cls_token"].expand(B, -1, -1), t], dim=1) + sd["pos_embed"]
        for i in range(c["depth"]):
            p = f"blocks.{i}."
            y = F.layer_norm(t, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
            qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
            N = qkv.shape[1]
            q, k, v = qkv.reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
            attn = ((q * 64 ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
            o = (attn @ v).transpose(1, 2).reshape(B, N, D)
            t = t + sd[p + "ls1.gamma"] * F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
            y = F.layer_norm(t, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
            h = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
            t = t + sd[p + "ls2.gamma"] * h
        want = F.layer_norm(t, (D,), sd["norm.weight"], sd["norm.bias"], 1e-6)[:, 0]
    assert torch.equal(got, want)


def _layout_rc(c):
    cfg = UniConfig(c["dim"], c["depth"], c["heads"], c["mlp_dim"], c["img"])
    return _lib.lib().sq_uni_layout_init(ctypes.byref(cfg), ctypes.byref(UniLayout()))


def test_refusals_restate_check_cfg():
    """Every row is admitted by the restated check and by the library's own, every refusal by neither, each by its message."""
    for c in uc.CASES:
        assert uc.admitted(c, MAX_DEPTH) and _layout_rc(c) == 0, c["id"]
        assert UniViT(**uc.model_kwargs(c)).cfg.mlp_dim == c["mlp_dim"]
    for r in uc.refusals(MAX_DEPTH):
        assert not uc.admitted(r, MAX_DEPTH), r["id"]
        assert _layout_rc(r) != 0, r["id"]
        with pytest.raises(_lib.SequoiaHipError, match=r["match"]):
            UniViT(**uc.model_kwargs(r))
    # the largest image size admitted is the table's largest: the next one is the first refusal
    assert uc.tokens(240) <= uc.MAX_TOKENS < uc.tokens(256)


def test_kernel_list_of_record_names_the_kernels_the_sweep_is_there_for():
    """profiles/uni_shape_contract_kernels.txt (the kernel trace of test_gpu_uni_shapes.py and test_gpu_uni_attn.py, reduced to
    names): passing is not enough if the dispatcher quietly took another kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "uni_shape_contract_kernels.txt")) as f:
        names = f.read()
    for want in ("uni_attn_kernel<float>", "uni_attn_mfma_kernel", "uni_attn_x3_kernel",
                 "uni_ln8_kernel<float, 2>", "uni_ln8_kernel<unsigned short, 2>", "uni_ln_kernel<float>", "uni_ln_kernel<unsigned short>",
                 "uni_ln8_x3_kernel<2>", "uni_ln_x3_kernel", "uni_im2col_kernel<float>", "uni_im2col_kernel<unsigned short>",
                 "uni_im2col_x3_kernel"):
        assert want in names, want
    assert "uni_attn_kernel<unsigned short>" not in names
