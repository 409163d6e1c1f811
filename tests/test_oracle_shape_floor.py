"""Is every row of tests/shape_cases.py a fair test?  (CPU only.)

The GPU sweep (test_gpu_shape_contract.py) holds the HIP path to 1e-4 (fp32 mode) and 3e-2 / 8e-2 / 2e-2 (bf16 mode:
predictions / gradient tensors / loss) of the float64 oracle.  That only means something if the reference alone sits
comfortably inside those bounds at the row's shape, and if the fp32 bound would catch the indexing and masking mistakes
the rows are there for.  Per row:

* the float32 oracle against the float64 oracle stays below 1e-5, a tenth of the fp32 tolerance;
* the whole oracle in CPU bfloat16 arithmetic (coarser than the HIP path's fp32 accumulators and fp32 master weights)
  against the float64 oracle stays below the bf16 tolerances (on shape_cases.ORACLE_THREADS threads: see oracle_threads);

and three kernel mistakes, restated as mutations of the oracle, each move a prediction or a gradient tensor by more than
1e-3 -- ten times the fp32 bound -- at the row that targets them."""
import os
import types

import pytest
import torch
import torch.nn.functional as F

import shape_cases as sc
from oracle import vis_oracle

IDS = [c["id"] for c in sc.ALL_CASES]


def _report(tag, case, t):
    line = f"{tag} {case['id']}: pred {t['pred']:.2e}"
    if "loss" in t:
        k, e = sc.worst_grad(t)
        line += f" loss {t['loss']:.2e} gx {t['gx']:.2e} worst gradient tensor {e:.2e} at {k}"
    print(line)


@pytest.mark.parametrize("case", sc.ALL_CASES, ids=IDS)
def test_float32_oracle_is_a_tenth_of_the_fp32_tolerance_from_float64(case):
    ref = sc.reference(case, torch.float64)
    t = sc.error_table(sc.reference(case, torch.float32), ref)
    _report("float32 oracle vs float64", case, t)
    assert t["pred"] < sc.FLOOR_F32
    if "loss" in t:
        assert t["loss"] < sc.FLOOR_F32 and t["gx"] < sc.FLOOR_F32
        bad = {k: e for k, e in t["grads"].items() if not e < sc.FLOOR_F32}
        assert not bad, bad


@pytest.mark.parametrize("case", sc.ALL_CASES, ids=IDS)
def test_bfloat16_oracle_is_inside_the_bf16_tolerances(case):
    ref = sc.reference(case, torch.float64)
    t = sc.error_table(sc.reference(case, torch.bfloat16), ref)
    _report("bfloat16 oracle vs float64", case, t)
    tol = sc.TOL["bf16"]
    assert t["pred"] < tol["pred"]
    if "loss" in t:
        assert t["loss"] < tol["loss"] and t["gx"] < tol["grad"]
        bad = {k: e for k, e in t["grads"].items() if not e < tol["grad"]}
        assert not bad, bad


# ---- teeth: what a subtly wrong kernel would do, as a mutation of the oracle, has to show at ten times the fp32 bound ----
TEETH = 1e-3


def _moved(case, monkeypatch, name, fn):
    ref = sc.reference(case, torch.float64)
    monkeypatch.setattr(vis_oracle, name, fn)
    t = sc.error_table(sc.reference_uncached(case, torch.float64), ref)
    monkeypatch.undo()
    k, e = sc.worst_grad(t)
    print(f"mutation at {case['id']}: predictions move by {t['pred']:.2e}, worst gradient tensor by {e:.2e} at {k}")
    return max(t["pred"], e)


def _attention_last_key_masked(sd, prefix, x, heads):
    """vis_oracle.vit_attention with the last key dropped from the softmax (a lane mask `j + 64 < N - 1`)."""
    D = x.shape[-1]
    y = F.layer_norm(x, (D,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"])
    qkv = F.linear(y, sd[prefix + "to_qkv.weight"]).chunk(3, dim=-1)
    B, N, inner = qkv[0].shape
    dh = inner // heads
    q, k, v = (t.reshape(B, N, heads, dh).permute(0, 2, 1, 3) for t in qkv)
    dots = torch.matmul(q, k.transpose(-1, -2)) * (dh ** -0.5)
    mask = torch.zeros(N, dtype=dots.dtype)
    mask[-1] = float("-inf")
    attn = torch.softmax(dots + mask, dim=-1)
    out = torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(B, N, inner)
    return F.linear(out, sd[prefix + "to_out.weight"])


def test_a_masked_last_key_would_show_at_n65(monkeypatch):
    case = sc.BY_ID["vit-D128-h2-F256-N65-L2-B3-G40"]
    assert _moved(case, monkeypatch, "vit_attention", _attention_last_key_masked) > TEETH


def _summary_of_slide_m_div_100(sd, prefix, x):
    """vis_oracle.summary_mixing with the summary term of token row m = b * N + n taken from slide m // 100 (instead of
    m // N = b): a row-bias index that is only right at the reference's N = 100."""
    f_dim = sd[prefix + "f.weight"].shape[0]
    s_dim = sd[prefix + "s.weight"].shape[0]
    B, N = x.shape[0], x.shape[1]
    local = F.linear(x, sd[prefix + "f.weight"], sd[prefix + "f.bias"])
    local = F.gelu(F.layer_norm(local, (f_dim,), sd[prefix + "local_norm.weight"], sd[prefix + "local_norm.bias"]))
    time = F.linear(x, sd[prefix + "s.weight"], sd[prefix + "s.bias"])
    time = F.gelu(F.layer_norm(torch.mean(time, dim=1), (s_dim,), sd[prefix + "summary_norm.weight"], sd[prefix + "summary_norm.bias"]))
    slide = (torch.arange(B * N) // 100) % B
    time = time[slide].reshape(B, N, s_dim)
    return F.gelu(F.linear(torch.cat([local, time], dim=-1), sd[prefix + "c.weight"], sd[prefix + "c.bias"]))


@pytest.mark.parametrize("cid", ["vis-D128-h2-L2-N7-B9-G40", "vis-D128-h2-L2-N300-B3-G40"])
def test_the_neighbouring_slides_summary_term_would_show_off_n100(monkeypatch, cid):
    assert _moved(sc.BY_ID[cid], monkeypatch, "summary_mixing", _summary_of_slide_m_div_100) > TEETH


def _functional_with_short_layer_norm():
    """torch.nn.functional with LayerNorm statistics over all but the last 1024 of 4096 columns (a row kernel whose per-lane
    register block is a quarter too short)."""
    def layer_norm(x, shape, weight=None, bias=None, eps=1e-5):
        if shape[0] != 4096:
            return F.layer_norm(x, shape, weight, bias, eps)
        head = x[..., :3072]
        mean = head.mean(dim=-1, keepdim=True)
        var = head.var(dim=-1, unbiased=False, keepdim=True)
        return (x - mean) / torch.sqrt(var + eps) * weight + bias
    ns = types.SimpleNamespace(**{k: getattr(F, k) for k in ("linear", "gelu", "mse_loss")})
    ns.layer_norm = layer_norm
    return ns


@pytest.mark.parametrize("cid", ["vis-D4096-h2-L1-N16-B3-G96", "vit-D4096-h2-F64-N16-L1-B3-G48"])
def test_layer_norm_statistics_that_miss_the_last_quarter_of_4096_columns_would_show(monkeypatch, cid):
    assert _moved(sc.BY_ID[cid], monkeypatch, "F", _functional_with_short_layer_norm()) > TEETH


def test_refused_rows_are_the_ones_the_launch_code_refuses():
    """The table's refusals restate the launch code's limits: ViS backward needs nheads a power of two; the ViT's attention
    backward keeps 4 * (257 N + N^2) bytes of one (slide, head) in 160 KiB of LDS."""
    for c in sc.VIS_CASES:
        assert (c["backward"] == sc.POW2) == (c["nheads"] & (c["nheads"] - 1) != 0), c["id"]
    for c in sc.VIT_CASES:
        assert (c["backward"] == sc.LDS) == (4 * (257 * c["N"] + c["N"] ** 2) > 160 * 1024), c["id"]
    for cid, rows in sc.GATHER_CASES:
        cache, members = sc.gather_inputs(sc.BY_ID[cid], rows)
        assert -1 <= int(members.min()) and int(members.max()) < cache.shape[0] and bool((members < 0).any())
    assert sc.BY_ID[sc.VIS_AFTER_REFUSAL]["backward"] == "ok" and sc.BY_ID[sc.VIT_AFTER_REFUSAL]["backward"] == "ok"


def test_kernel_list_of_record_names_the_shape_selected_instantiations():
    """profiles/shape_contract_kernels.txt (the kernel trace of test_gpu_shape_contract.py, reduced to names): passing is not
    enough if the dispatcher quietly took another kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "shape_contract_kernels.txt")) as f:
        names = f.read()
    for want in ("ln_rows_kernel<16, false>", "ln_rows_kernel<16, true>", "ln_rows_kernel<8, true>", "ln_rows_bwd_kernel<8, ",
                 "ln_rows_bwd_kernel<16, ", "ln_rows_bwd_lean_kernel<4>", "ln_rows_bwd_lean_kernel<8>", "ln64_gelu_bwd_kernel<2, ",
                 "ln64_gelu_bwd_kernel<4, ", "ln64_gelu_bwd_lean_kernel<", "attn_fwd_kernel<float>", "attn_fwd_kernel<unsigned short>",
                 "attn_bwd_kernel<float>", "attn_bwd_kernel<unsigned short>", "colsum_multi_kernel", "colsum_stage1<", "colsum_stage2",
                 "gemm_p8_kernel<13, ",      # LayerNorm(64) + GELU + the ViS combiner in the f projection's epilogue
                 "summary_fwd_kernel", "token_mean_bf16x8_kernel", "add_pos_gather_kernel", "group_sum4_kernel<", "bcast_rows_kernel"):
        assert want in names, want
