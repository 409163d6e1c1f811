"""The HE2RNA training step on the device (csrc/he2rna_train.hip, sequoia_pub_amd.he2rna.He2rnaTrainStep, fit(engine="fused"),
cli/he2rna.py) against the existing entries, the float64 reference of tests/he2rna_train_cases.py and the autograd path.

Bounds: the project's fp32 bound of tests/test_gpu_he2rna.py -- 1e-4 relative, atol = 1e-4 * max|ref| per tensor.  On the CPU torch
in float32 follows the float64 reference over these 12 steps within 1.6e-7 (loss, relative) and 1.5e-7 (parameters, absolute)."""
import os
import pickle
import sys

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import he2rna_train_cases as tc  # noqa: E402
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, evalstats, store  # noqa: E402
from sequoia_pub_amd import he2rna as he  # noqa: E402
from sequoia_pub_amd.cli import he2rna as cli  # noqa: E402
from sequoia_pub_amd.he2rna import HE2RNA, He2rnaTrainStep  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _assert_close(got, ref, what):
    """|got - ref| <= 1e-4 * max|ref| + 1e-4 * |ref| elementwise (rtol 1e-4, atol 1e-4 max|ref|)."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    bound = 1e-4 * ref.abs().max() + 1e-4 * ref.abs()
    assert bool(((got - ref).abs() <= bound).all()), (what, _rel(got, ref))


# ---------------------------------------------------------------------------------------------------------------------
# 1. loss head against sq_he2rna_topk_mean + sq_mse_loss_grad + sq_he2rna_topk_mean_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _head_inputs(B, N, G, seed, first_masked=False):
    g = torch.Generator().manual_seed(seed)
    ld = tc.up8(G) + 8                                                      # over-allocated rows
    scores = torch.round(torch.randn(B, N, ld, generator=g) * 6) / 4        # multiples of 0.25: exact ties in every long column
    mask = torch.ones(B, N)
    if N >= 7:
        mask[0, N // 2] = 0
        mask[0, N - 1] = 0
        mask[B - 1, N - 3:] = 0
    if first_masked:
        mask[B - 1, 0] = 0
    target = torch.rand(B, G, generator=g) * 3
    return scores.to(DEV), mask.to(DEV), target.to(DEV), ld


def _three_entries(scores, ld, mask, ks, scale, target, gscale, B, N, G, want_grad=True):
    lib, st = _lib.lib(), _lib.stream_ptr(DEV)
    ks = np.asarray(ks, dtype=np.int32)
    pred = torch.empty(B, G, device=DEV)
    _lib.check(lib.sq_he2rna_topk_mean(_lib.ptr(scores), ld, _lib.ptr(mask), ks.ctypes.data, len(ks), scale, _lib.ptr(pred), B, N, G, st))
    if not want_grad:
        return pred, None, None
    gout, loss = torch.empty(B, G, device=DEV), torch.empty(1, device=DEV)
    scratch = torch.empty(lib.sq_train_scratch_bytes(G), dtype=torch.uint8, device=DEV)
    _lib.check(lib.sq_mse_loss_grad(_lib.ptr(pred), _lib.ptr(target), B * G, gscale, _lib.ptr(gout), _lib.ptr(loss), _lib.ptr(scratch), st))
    grad = torch.full((B, N, ld), SENTINEL, device=DEV)
    _lib.check(lib.sq_he2rna_topk_mean_bwd(_lib.ptr(scores), ld, _lib.ptr(mask), ks.ctypes.data, len(ks), scale, _lib.ptr(gout), _lib.ptr(grad),
                                           ld, B, N, G, st))
    return pred, loss, grad


def _loss_head(scores, ld, mask, ks, scale, target, gscale, B, N, G, want_grad=True):
    lib, st = _lib.lib(), _lib.stream_ptr(DEV)
    ks = np.asarray(ks, dtype=np.int32)
    pred, loss = torch.empty(B, G, device=DEV), torch.empty(1, device=DEV)
    grad = torch.full((B, N, ld), SENTINEL, device=DEV) if want_grad else None
    ws = torch.empty(lib.sq_he2rna_loss_head_workspace_bytes(B, G), dtype=torch.uint8, device=DEV)
    _lib.check(lib.sq_he2rna_loss_head(_lib.ptr(scores), ld, _lib.ptr(mask), ks.ctypes.data, len(ks), scale, _lib.ptr(target), gscale,
                                       _lib.ptr(pred), _lib.ptr(loss), _lib.ptr(grad), ld, B, N, G, _lib.ptr(ws), ws.numel(), st))
    return pred, loss, grad


def _check_head(B, N, G, ks, scale, seed):
    scores, mask, target, ld = _head_inputs(B, N, G, seed)
    gscale = 2.0 / (B * G)
    ref = _three_entries(scores, ld, mask, ks, scale, target, gscale, B, N, G)
    got = _loss_head(scores, ld, mask, ks, scale, target, gscale, B, N, G)
    tag = (B, N, G, ks)
    assert bool(torch.isfinite(ref[0]).all()) and torch.equal(got[0], ref[0]), tag
    assert torch.equal(got[2][:, :, :G], ref[2][:, :, :G]) and bool((got[2][:, :, G:] == SENTINEL).all()), tag
    assert float(ref[2][:, :, :G].abs().max()) > 0
    assert abs(float(got[1]) - float(ref[1])) <= 1e-6 * abs(float(ref[1])), (tag, float(got[1]), float(ref[1]))


@pytest.mark.parametrize("N", [1, 7, 100, 128])
def test_loss_head_equals_the_three_entries_bit_for_bit(N):
    """pred and grad_scores[:, :, :G] bit-equal, loss within 1e-6, columns >= G of the sentinel-filled gradient table unchanged:
    G in {1, 12, 203}, B in {1, 3}, k in {1, N}, and the seven-k mean where 100 tiles allow it; scores with exact ties, tiles masked
    in the middle and at the end."""
    _lib.require_gpu()
    seed = 100 * N
    for G in (1, 12, 203):
        for B in (1, 3):
            for ks, scale in [([1], 1.0), ([N], 1.0)] + ([(tc.ALL_KS, 1.0 / 7)] if N >= 100 else []):
                seed += 1
                _check_head(B, N, G, ks, scale, seed)


def test_loss_head_at_the_experiment_gene_count():
    _lib.require_gpu()
    _check_head(2, 100, 20820, [10], 1.0, 77)


def test_loss_head_forward_only_reproduces_the_nan_of_a_masked_first_tile():
    _lib.require_gpu()
    B, N, G = 3, 20, 12
    scores, mask, target, ld = _head_inputs(B, N, G, 5, first_masked=True)
    ref, _, _ = _three_entries(scores, ld, mask, [1], 1.0, target, 1.0, B, N, G, want_grad=False)
    got, loss, _ = _loss_head(scores, ld, mask, [1], 1.0, target, 1.0, B, N, G, want_grad=False)
    assert bool(torch.isnan(ref[B - 1]).all()) and not bool(torch.isnan(ref[:B - 1]).any())
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[:B - 1], ref[:B - 1]) and bool(torch.isnan(loss).all())


def test_loss_head_refuses_what_he2rna_hip_refuses():
    _lib.require_gpu()
    scores, mask, target, ld = _head_inputs(1, 7, 12, 1)
    with pytest.raises(_lib.SequoiaHipArgError, match="k=8 out of range"):
        _loss_head(scores, ld, mask, [8], 1.0, target, 1.0, 1, 7, 12)
    with pytest.raises(_lib.SequoiaHipArgError, match="129 tiles"):
        _loss_head(scores, ld, mask, [1], 1.0, target, 1.0, 1, 129, 12)


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. trajectories
# ---------------------------------------------------------------------------------------------------------------------
def _model(name, dropout=0.0):
    c, sd, batches = tc.case(name)
    m = HE2RNA(input_dim=c["D"], output_dim=c["G"], layers=c["layers"], ks=c["ks"], dropout=dropout, device=DEV)
    m.load_state_dict(sd)
    return c, sd, batches, m


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_fused_trajectory_follows_the_float64_reference(name):
    _lib.require_gpu()
    c, sd, batches, m = _model(name)
    ref_losses, ref_final, ref_first = tc.reference_trajectory(name)
    tr = He2rnaTrainStep(m, tc.LR)
    m.train()
    np.random.seed(tc.K_SEED)
    losses, worst_g = [], 0.0
    for t in range(tc.STEPS):
        x, y = batches[t % 3]
        losses.append(tr.step(x, y))
        if t == 0:
            for n, g in tr.grad_views().items():
                worst_g = max(worst_g, _rel(g.double().cpu(), ref_first[n]))
                _assert_close(g, ref_first[n], (name, "gradient", n))
    losses = [float(v) for v in torch.stack(losses).cpu()]
    worst_l = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_losses))
    views = tr.param_views()
    worst_p = max(_rel(views[n].double().cpu(), ref_final[n]) for n in views)
    print(f"HE2RNA fused step {name}: worst loss rel err {worst_l:.2e}, gradient (step 1) {worst_g:.2e}, parameters (step 12) {worst_p:.2e}")
    assert worst_l <= 1e-4, (losses, ref_losses)
    for n, v in views.items():
        assert float((v.double().cpu() - ref_final[n]).abs().max()) <= 1e-4 * float(ref_final[n].abs().max()), n
    pad = tr.padding_mask()
    assert int(pad.sum()) == tr.total - sum(v.numel() for v in ref_final.values())
    for buf in (tr.flat, tr.exp_avg, tr.exp_avg_sq, tr.grad):
        assert bool((buf[pad] == 0).all())
    assert float(tr.exp_avg_sq.max()) > 0
    state = m.state_dict()
    assert list(state) == list(sd)
    for n, v in views.items():
        assert state[n].shape == sd[n].shape and torch.equal(state[n], v) and not torch.equal(state[n].cpu(), sd[n])


def test_fused_and_autograd_losses_agree_on_the_device():
    _lib.require_gpu()
    c, sd, batches, m_auto = _model("mid")
    m_auto.train()
    opt = torch.optim.Adam(list(m_auto.parameters()), lr=tc.LR, weight_decay=0.0)
    np.random.seed(tc.K_SEED)
    auto = []
    for t in range(tc.STEPS):
        x, y = batches[t % 3]
        loss = torch.nn.functional.mse_loss(m_auto(x.to(DEV).transpose(1, 2)), y.to(DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()
        auto.append(float(loss.detach()))
    _, _, _, m_fused = _model("mid")
    m_fused.train()
    tr = He2rnaTrainStep(m_fused, tc.LR)
    np.random.seed(tc.K_SEED)
    fused = [float(v) for v in torch.stack([tr.step(*batches[t % 3]) for t in range(tc.STEPS)]).cpu()]
    worst = max(abs(a - b) / abs(b) for a, b in zip(fused, auto))
    print(f"HE2RNA fused vs autograd on the device, 12 losses: worst rel diff {worst:.2e}")
    assert worst <= 1e-4, (fused, auto)


# ---------------------------------------------------------------------------------------------------------------------
# 4. dropout
# ---------------------------------------------------------------------------------------------------------------------
def _hidden_reference(sd, x, acts, c):
    """Per hidden layer: the float64 pre-dropout activation ReLU(conv(input)) as [B * N, width], layer i fed the SAVED (post-dropout)
    activation of layer i - 1."""
    out = []
    h = x.double()[:, :, c["C"] - c["D"]:].reshape(c["B"] * c["N"], c["D"])
    for i in range(len(c["layers"])):
        w, b = sd[f"conv{i}.weight"].double().squeeze(-1), sd[f"conv{i}.bias"].double()
        out.append(torch.relu(h @ w.t() + b))
        h = acts[i].double().cpu()
    return out


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_dropout_is_counter_based_scaled_and_replayable(name):
    _lib.require_gpu()
    p = 0.5
    c, sd, batches, m = _model(name, dropout=p)
    x, y = batches[0]
    tr = He2rnaTrainStep(m, tc.LR, seed=1234)
    k = c["ks"][1]
    tr.step_index = 3
    loss = tr.forward_backward(x, y, k)
    acts = tr.saved_activations()
    grads = {n: g.clone() for n, g in tr.grad_views().items()}
    refs = _hidden_reference(sd, x, acts, c)
    for i, (a, h) in enumerate(zip(acts, refs)):
        a = a.double().cpu()
        active = h > 1e-4
        n = int(active.sum())
        kept = int((a[active] > 0).sum())
        assert n > 0 and abs(kept - p * n) <= 5 * (n * p * (1 - p)) ** 0.5, (name, i, kept, n)
        on = active & (a > 0)
        assert float((a[on] - 2 * h[on]).abs().max()) <= 1e-4 * float(h.abs().max()), (name, i)
    # the same (seed, step index): the same bits; the next step index: another pattern
    tr.forward_backward(x, y, k)
    again = tr.saved_activations()
    assert all(torch.equal(a, b) for a, b in zip(acts, again))
    tr.step_index = 4
    tr.forward_backward(x, y, k)
    a0, b0 = acts[0].cpu(), tr.saved_activations()[0].cpu()
    active = refs[0] > 1e-4
    changed = float(((a0 > 0) != (b0 > 0))[active].double().mean())
    # expected 0.5; `mid` (thousands of units) must exceed 0.4 outright, the 60- and 300-unit tail cases get 2.5 binomial sigmas more
    assert changed > (0.4 if int(active.sum()) >= 400 else 0.4 - 2.5 * (0.25 / int(active.sum())) ** 0.5), (name, changed)
    # gradient: float64 autograd through the oracle, replayed with the gate (a > 0) / (1 - p)
    ref_loss, ref_grads = tc.loss_and_grads(sd, x, y, k, c["D"], gates=[tc.replay_gate(a.double().cpu(), p) for a in acts])
    assert abs(float(loss) - ref_loss) <= 1e-4 * abs(ref_loss)
    for n, g in grads.items():
        _assert_close(g, ref_grads[n], (name, "dropout gradient", n))


def test_dropout_p0_is_the_dropout_free_path_and_p1_is_refused():
    _lib.require_gpu()
    c, sd, batches, m = _model("l5x12", dropout=0.0)
    x, y = batches[0]
    xt = x.to(DEV).reshape(c["B"] * c["N"], c["C"]).contiguous()
    stack, _ = he._layer_stack(xt, m)
    tr = He2rnaTrainStep(m, tc.LR)
    tr.forward_backward(x, y, 5)
    for a, b, width in zip(tr.saved_activations(), stack[1:-1], c["layers"]):
        assert torch.equal(a, b[:, :width])
    buf = torch.rand(7, 16, device=DEV)
    before = buf.clone()
    _lib.check(_lib.lib().sq_he2rna_dropout(_lib.ptr(buf), 16, 7, 13, 0.0, 1, 0, 0, _lib.stream_ptr(DEV)))
    assert torch.equal(buf, before)
    _lib.check(_lib.lib().sq_he2rna_dropout(_lib.ptr(buf), 16, 7, 13, 0.5, 1, 0, 0, _lib.stream_ptr(DEV)))
    assert torch.equal(buf[:, 13:], before[:, 13:]) and bool(((buf[:, :13] == 0) | (buf[:, :13] == 2 * before[:, :13])).all())
    assert 0 < int((buf[:, :13] == 0).sum()) < 7 * 13
    with pytest.raises(_lib.SequoiaHipArgError, match="p = 1 must be in"):
        _lib.check(_lib.lib().sq_he2rna_dropout(_lib.ptr(buf), 16, 7, 13, 1.0, 1, 0, 0, _lib.stream_ptr(DEV)))
    m.p_drop = 1.0
    with pytest.raises(_lib.SequoiaHipArgError, match="p = 1 must be in"):
        tr.forward_backward(x, y, 5)


# ---------------------------------------------------------------------------------------------------------------------
# 5. full size
# ---------------------------------------------------------------------------------------------------------------------
def test_full_size_step_matches_the_autograd_path():
    """B = 16, N = 100, D = 2048, layers [256, 256], G = 20 820, dropout 0, k = 10: gradient and loss of the fused passes against the
    existing autograd path on the device (no CPU oracle at this size)."""
    _lib.require_gpu()
    B, N, D, G = 16, 100, 2048, 20820
    torch.manual_seed(9)
    m = HE2RNA(input_dim=D, output_dim=G, layers=[256, 256], ks=tc.ALL_KS, dropout=0.0, device=DEV)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(B, N, D, generator=g).clamp_min(-0.2)
    x[0, 80:] = 0
    x[1, 40] = 0
    y = torch.rand(B, G, generator=g) * 3
    m.train()
    loss = torch.nn.functional.mse_loss(m.forward_fixed_k(x.to(DEV).transpose(1, 2), 10), y.to(DEV))
    loss.backward()
    ref = {n: g.clone() for n, g in m.grad_views(m.flat.grad).items()}
    tr = He2rnaTrainStep(m, 1e-3)
    got = tr.forward_backward(x, y, 10)
    assert abs(float(got) - float(loss.detach())) <= 1e-4 * abs(float(loss.detach()))
    for n, gv in tr.grad_views().items():
        assert float(ref[n].abs().max()) > 0
        _assert_close(gv, ref[n], ("full size", n))


# ---------------------------------------------------------------------------------------------------------------------
# 6. validation score on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 37])
@pytest.mark.parametrize("G", [1, 50, 1031])
def test_device_validation_score_equals_compute_correlations(n, G):
    _lib.require_gpu()
    g = torch.Generator().manual_seed(n * 10000 + G)
    labels = torch.rand(n, G, generator=g) * 3
    pred = labels * 0.5 + torch.randn(n, G, generator=g)                   # negative predictions: the ReLU matters
    if G == 1:
        pred[:, 0] = torch.tensor([0.5, -0.25] + [0.1 * i for i in range(n - 2)])      # varies after the ReLU: r is finite
    assert bool((pred < 0).any())
    if G > 1:
        labels[:, G // 2] = 1.25                                            # a constant label column: skipped
        pred[:, G // 3] = -0.5                                              # constant after the ReLU: NaN r, dropped
    ref = he.compute_correlations(labels.numpy(), torch.relu(pred).numpy())
    got = float(he.device_validation_score(pred.to(DEV), labels.to(DEV)))
    assert np.isfinite(ref) and abs(got - ref) <= 1e-6, (got, ref)


def test_device_validation_score_is_nan_when_no_gene_is_left():
    _lib.require_gpu()
    labels, pred = torch.full((1, 5), 2.0), torch.rand(1, 5)
    assert np.isnan(float(he.device_validation_score(pred.to(DEV), labels.to(DEV))))


# ---------------------------------------------------------------------------------------------------------------------
# 7. the experiment script end to end
# ---------------------------------------------------------------------------------------------------------------------
def _cohort(root, n_genes, name):
    rs = np.random.RandomState(4)
    rows = []
    for i in range(10):
        slide = f"TCGA-AA-{i:04d}"
        d = os.path.join(root, "features", "TCGA-BRCA", slide)
        if not os.path.exists(d):
            os.makedirs(d)
            with store.File(os.path.join(d, slide + ".h5"), "w") as f:
                f.create_dataset("cluster_features", data=rs.rand(100, 32).astype(np.float32))
        rows.append(dict(wsi_file_name=slide, patient_id=f"P{i}", tcga_project="TCGA-BRCA",
                         **{f"rna_G{g}": float(rs.rand() * 6) for g in range(n_genes)}))
    path = os.path.join(root, name)
    pd.DataFrame(rows).to_csv(path, index=False)
    return path


def _check_outputs(out, n_genes):
    res = pickle.load(open(os.path.join(out, "test_results.pkl"), "rb"))
    assert set(res) == {f"split_{i}" for i in range(5)} | {"genes"} and len(res["genes"]) == n_genes
    for i in range(5):
        s = res[f"split_{i}"]
        assert set(s) == {"real", "preds", "random", "wsi_file_name", "tcga_project"}
        assert s["preds"].shape == (2, n_genes) and s["random"].shape == (2, n_genes) and s["real"].shape == (2, n_genes)
        assert (s["preds"] >= 0).all() and (s["random"] >= 0).all() and not np.array_equal(s["preds"], s["random"])
        m = torch.load(os.path.join(out, f"model_{i}.pt"), weights_only=False)
        assert isinstance(m, HE2RNA) and tuple(m.state_dict()["conv2.weight"].shape) == (n_genes, 256, 1)
    return res


def test_experiment_script_end_to_end(tmp_path):
    _lib.require_gpu()
    root = str(tmp_path)
    csv24 = _cohort(root, 24, "ref24.csv")
    common = ["--feature_path", os.path.join(root, "features"), "--k", "5", "--batch_size", "4", "--max_epochs", "2", "--patience", "5",
              "--log", "0", "--destfolder", root, "--subfolder", "he2rna"]
    cli.main(["--path_csv", csv24, "--exp_name", "fused", "--engine", "fused"] + common)
    out = os.path.join(root, "he2rna", "fused")
    res = _check_outputs(out, 24)
    stats = evalstats.evaluate_test_results(res, folds=5)
    assert len(stats) > 0
    cli.main(["--path_csv", _cohort(root, 30, "ref30.csv"), "--exp_name", "finetune", "--engine", "fused", "--checkpoint",
              os.path.join(out, "model_0.pt"), "--change_num_genes", "--num_genes", "24"] + common)
    _check_outputs(os.path.join(root, "he2rna", "finetune"), 30)
    cli.main(["--path_csv", csv24, "--exp_name", "autograd", "--engine", "autograd"] + common)
    _check_outputs(os.path.join(root, "he2rna", "autograd"), 24)
