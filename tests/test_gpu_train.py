"""ViS backward / MSE / AdamW / metrics / train loop on the HIP path vs reference golden vectors
(tests/golden/vis_tiny.npz, metrics_train.npz) and the CPU oracle."""
import os

import numpy as np
import pytest
import torch

from gpu_util import assert_allclose_rel, rel_err

pytestmark = pytest.mark.gpu

from oracle import metrics_oracle, vis_oracle  # noqa: E402  (checker only)
from sequoia_pub_amd import _lib, synth  # noqa: E402
from sequoia_pub_amd import train as sq_train  # noqa: E402
from sequoia_pub_amd.vis import ViS  # noqa: E402

TINY = dict(num_outputs=50, input_dim=128, depth=2, nheads=2, dimensions_f=64, dimensions_s=64, dimensions_c=64)


def _tiny(golden_dir, mode="fp32"):
    z = np.load(os.path.join(golden_dir, "vis_tiny.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w::")}
    m = ViS(**TINY, device="cuda:0", compute_dtype=mode)
    m.load_state_dict(sd)
    m.to("cuda:0")
    return z, sd, m


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-4), ("bf16", 6e-2)])
def test_grads_match_reference_autograd(golden_dir, mode, tol):
    _lib.require_gpu()
    z, sd, m = _tiny(golden_dir, mode)
    x = torch.from_numpy(z["x"]).cuda().requires_grad_(True)
    y = torch.from_numpy(z["target"]).cuda()
    pred = m(x)
    loss, gpred = sq_train.mse_loss_grad(m, pred.detach(), y)
    assert abs(float(loss) - float(z["loss"])) < (1e-5 if mode == "fp32" else 2e-2) * float(z["loss"])
    pred.backward(gpred)
    gv = m.grad_views(m.flat.grad)
    worst = ("", 0.0)
    for k in (k for k in z.files if k.startswith("g::")):
        e = rel_err(gv[k[3:]].cpu().numpy(), z[k])
        if e > worst[1]:
            worst = (k, e)
    print(f"grads {mode}: worst per-tensor rel err {worst[1]:.3e} at {worst[0]}")
    assert worst[1] < tol, worst
    # gradient w.r.t. the input tokens against the oracle
    xo = torch.from_numpy(z["x"]).requires_grad_(True)
    torch.nn.functional.mse_loss(vis_oracle.vis_forward(sd, xo), torch.from_numpy(z["target"])).backward()
    assert rel_err(x.grad.cpu().numpy(), xo.grad.numpy()) < tol


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-4), ("bf16", 6e-2)])
def test_grads_with_mixed_gradient_shapes_and_grouped_launches(mode, tol, monkeypatch):
    """nheads * 64 != input_dim: the four large weight gradients of a layer have three different shapes, so the per-layer
    grouped launch (vis_bwd.hip: same-shape members share one TN launch) splits into a pair and two singles.  Every tensor
    against the oracle's autograd, and the grouped path against one launch per gradient (SQ_BWD_NO_GROUP=1)."""
    _lib.require_gpu()
    cfg = dict(num_outputs=72, input_dim=192, depth=2, nheads=2, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    sd = vis_oracle.perturb_norm_params(vis_oracle.init_vis_state_dict(**cfg, seed=21), seed=22)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 100, 192, generator=g)
    y = torch.rand(5, 72, generator=g) * 8
    loss_ref, _, grads_ref = vis_oracle.vis_loss_and_grads(sd, x, y)

    def grads(no_group):
        if no_group:
            monkeypatch.setenv("SQ_BWD_NO_GROUP", "1")
        else:
            monkeypatch.delenv("SQ_BWD_NO_GROUP", raising=False)
        m = ViS(**cfg, device="cuda:0", compute_dtype=mode)
        m.load_state_dict(sd)
        m.to("cuda:0")
        pred = m(x.cuda())
        loss, gpred = sq_train.mse_loss_grad(m, pred.detach(), y.cuda())
        pred.backward(gpred)
        torch.cuda.synchronize()
        return m, m.flat.grad.detach().clone(), float(loss)
    m, grouped, loss = grads(False)
    _, single, _ = grads(True)
    assert rel_err(grouped.cpu().numpy(), single.cpu().numpy()) < 1e-5      # same products; the K slicing (fp32 summation order) may differ
    gv = m.grad_views(grouped)
    worst = max(((k, rel_err(gv[k].cpu().numpy(), v.numpy())) for k, v in grads_ref.items()), key=lambda t: t[1])
    print(f"grads (D=192, 2 heads) {mode}: worst per-tensor rel err {worst[1]:.3e} at {worst[0]}")
    assert worst[1] < tol, worst
    assert abs(loss - float(loss_ref)) < (1e-5 if mode == "fp32" else 2e-2) * float(loss_ref)


def test_three_fused_adamw_steps_match_reference(golden_dir):
    _lib.require_gpu()
    z, sd, m = _tiny(golden_dir)
    x, y = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["target"]).cuda()
    stepper = sq_train.FusedTrainStep(m, lr=1e-3)
    losses = [float(stepper.step(x, y)[0]) for _ in range(3)]
    np.testing.assert_allclose(losses, z["losses3"], rtol=1e-4)
    after = m.state_dict()
    for k in (k for k in z.files if k.startswith("w3::")):
        np.testing.assert_allclose(after[k[4:]].cpu().numpy(), z[k], rtol=1e-3, atol=3e-5, err_msg=k)


def test_bucketed_overlapped_allreduce_path_matches(golden_dir, monkeypatch):
    """The data-parallel step (per-bucket events recorded mid-backward, all-reduce on a side stream) on a
    one-rank RCCL group must reproduce the plain step bit for bit."""
    _lib.require_gpu()
    import torch.distributed as dist
    z, sd, m = _tiny(golden_dir)
    x, y = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["target"]).cuda()
    plain = sq_train.FusedTrainStep(m, lr=1e-3)
    ref_losses = [float(plain.step(x, y)[0]) for _ in range(3)]
    ref_flat = m.flat.detach().clone()
    z, sd, m2 = _tiny(golden_dir)
    monkeypatch.setenv("SQ_FORCE_BUCKETS", "1")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29533", rank=0, world_size=1)
        created = True
    try:
        st = sq_train.FusedTrainStep(m2, lr=1e-3)
        assert st.overlap and len(st.buckets) == m2.cfg.depth + 1
        losses = [float(st.step(x, y)[0]) for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        if created:
            dist.destroy_process_group()
    assert losses == ref_losses
    assert torch.equal(m2.flat.detach(), ref_flat)


def test_torch_optimizer_through_autograd_matches_fused(golden_dir):
    _lib.require_gpu()
    z, sd, m = _tiny(golden_dir)
    x, y = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["target"]).cuda()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, amsgrad=False, weight_decay=0.0)   # main.py:180-183
    for _ in range(3):
        pred = m(x)
        loss, gpred = sq_train.mse_loss_grad(m, pred.detach(), y)
        opt.zero_grad()
        pred.backward(gpred)
        opt.step()
    after = m.state_dict()
    for k in (k for k in z.files if k.startswith("w3::")):
        np.testing.assert_allclose(after[k[4:]].cpu().numpy(), z[k], rtol=1e-3, atol=3e-5, err_msg=k)


def test_batch_metrics_match_reference(golden_dir):
    _lib.require_gpu()
    z = np.load(os.path.join(golden_dir, "metrics_train.npz"))
    m = ViS(300, 64, 1, 1, 64, 64, 64, device="cuda:0").to("cuda:0")
    out = sq_train.batch_metrics(m, torch.from_numpy(z["preds"]).cuda(), torch.from_numpy(z["labels"]).cuda()).cpu().numpy()
    assert abs(out[0] - float(z["mae"])) < 1e-6 * float(z["mae"]) + 1e-6
    assert abs(out[1] - float(z["corr"])) < 1e-6
    assert int(out[2]) == 298                      # 300 genes - 1 constant target - 1 NaN (constant prediction)
    loss, _ = sq_train.mse_loss_grad(m, torch.from_numpy(z["preds"]).cuda(), torch.from_numpy(z["labels"]).cuda(), want_grad=False)
    assert abs(float(loss) - float(z["mse"])) < 1e-5 * float(z["mse"])


def test_metrics_full_size_vs_oracle():
    _lib.require_gpu()
    y = synth.rna_targets(3, 64)
    p = (y + np.random.RandomState(1).randn(*y.shape)).astype(np.float32)
    m = ViS(20820, 64, 1, 1, 64, 64, 64, device="cuda:0").to("cuda:0")
    out = sq_train.batch_metrics(m, torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()).cpu().numpy()
    assert abs(out[1] - metrics_oracle.compute_correlations_vectorised(y, p)) < 1e-6
    assert abs(out[0] - metrics_oracle.mean_absolute_error(y, p)) < 1e-5


def test_train_loop_trace_matches_reference(golden_dir, tmp_path):
    """vit.py:117-243 on the tiny model: per-epoch losses of the reference run (make_golden.py)."""
    _lib.require_gpu()
    z = np.load(os.path.join(golden_dir, "metrics_train.npz"))
    sd = vis_oracle.init_vis_state_dict(**TINY, seed=21)
    m = ViS(**TINY, device="cuda:0")
    m.load_state_dict(sd)
    m.to("cuda:0")
    g = torch.Generator().manual_seed(13)
    xs = torch.randn(12, 100, 128, generator=g)
    ys = torch.rand(12, 50, generator=g) * 8
    names = [f"w{i}" for i in range(12)]

    def loader(lo, hi, bs=4):
        return [(xs[i:i + bs], ys[i:i + bs], names[i:i + bs], ["P"] * len(names[i:i + bs])) for i in range(lo, hi, bs)]
    loaders = {"train": loader(0, 8), "val": loader(8, 12)}
    import contextlib, io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m = sq_train.train(m, loaders, None, num_epochs=4, save_dir=str(tmp_path / "exp"), patience=20, split=None)
        preds, real, wsis, projs = sq_train.evaluate(m, loaders["val"], verbose=False)
        preds_p, wsis_p, _ = sq_train.predict(m, loaders["val"])
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("Epoch")]
    tr = [float(l.split("loss")[1].split("mae")[0]) for l in lines]
    mae = [float(l.split("mae")[1]) for l in lines]
    np.testing.assert_allclose(tr, z["train_epoch_loss"], rtol=2e-4)
    np.testing.assert_allclose(mae, z["train_epoch_mae"], rtol=2e-4)
    assert rel_err(preds, z["eval_preds"]) < 1e-3 and rel_err(preds_p, z["predict_preds"]) < 1e-3
    assert list(wsis) == list(z["eval_wsis"])
    assert os.path.exists(tmp_path / "exp" / "model_best.pt")          # split None/0 -> no suffix (vit.py:124)
    ck = torch.load(tmp_path / "exp" / "model_best.pt")
    assert set(ck.keys()) == set(sd.keys())


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-4), ("bf16", 8e-2)])
def test_full_size_grads_vs_oracle(mode, tol):
    """BASELINE config-2 model (D=1024, 6 layers, 16 heads, G=20820), B=2, against CPU autograd."""
    _lib.require_gpu()
    cfg = dict(num_outputs=20820, input_dim=1024, depth=6, nheads=16, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    sd = vis_oracle.perturb_norm_params(vis_oracle.init_vis_state_dict(**cfg, seed=99), seed=5)
    x = torch.from_numpy(synth.cluster_tokens(99, 2, 1024))
    y = torch.from_numpy(synth.rna_targets(7, 2))
    torch.set_num_threads(min(32, os.cpu_count()))
    loss_ref, _, grads_ref = vis_oracle.vis_loss_and_grads(sd, x, y)
    m = ViS(**cfg, device="cuda:0", compute_dtype=mode)
    m.load_state_dict(sd)
    m.to("cuda:0")
    pred = m(x.cuda())
    loss, gpred = sq_train.mse_loss_grad(m, pred.detach(), y.cuda())
    pred.backward(gpred)
    gv = m.grad_views(m.flat.grad)
    worst = ("", 0.0)
    for k, gr in grads_ref.items():
        e = rel_err(gv[k].cpu().numpy(), gr.numpy())
        if e > worst[1]:
            worst = (k, e)
    print(f"full-size grads {mode}: worst per-tensor rel err {worst[1]:.3e} at {worst[0]}; loss {float(loss):.5f} vs {float(loss_ref):.5f}")
    assert worst[1] < tol, worst


def test_full_size_batch64_bf16_step_vs_oracle():
    """Exactly what bench.py's vis_train workload times -- the BASELINE config-2 model, batch 64, bf16 mode, forward +
    MSE + backward -- against CPU fp32 autograd: loss, predictions and a subset of gradient tensors of every layer
    (all of layer 0 and of the head, projection / FF / one mixer of the others)."""
    _lib.require_gpu()
    cfg = dict(num_outputs=20820, input_dim=1024, depth=6, nheads=16, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    sd = vis_oracle.perturb_norm_params(vis_oracle.init_vis_state_dict(**cfg, seed=99), seed=5)
    B = 64
    x = torch.from_numpy(synth.cluster_tokens(99, B, 1024))
    y = torch.from_numpy(synth.rna_targets(7, B))
    torch.set_num_threads(min(32, os.cpu_count()))
    loss_ref, pred_ref, grads_ref = vis_oracle.vis_loss_and_grads(sd, x, y)
    m = ViS(**cfg, device="cuda:0", compute_dtype="bf16")
    m.load_state_dict(sd)
    m.to("cuda:0")
    pred = m._run_forward(x.cuda(), save=True)
    loss, gpred = sq_train.mse_loss_grad(m, pred, y.cuda())
    gflat, _ = sq_train.vis_backward(m, gpred, B, False)
    gv = m.grad_views(gflat)
    e_pred = rel_err(pred.cpu().numpy(), pred_ref.detach().numpy())
    assert_allclose_rel(pred.cpu().numpy(), pred_ref.detach().numpy(), 2e-2, "bf16 predictions at B=64")
    keys = [k for k in grads_ref if k.startswith("transformer.layers.0.") or k.startswith("linear_head") or k == "pos_emb1D"
            or ".mixers.7." in k or ".projection." in k or ".1.net." in k]
    assert len(keys) > 100
    worst = ("", 0.0)
    for k in keys:
        e = rel_err(gv[k].cpu().numpy(), grads_ref[k].numpy())
        if e > worst[1]:
            worst = (k, e)
    print(f"B=64 bf16 step: pred rel err {e_pred:.3e}; loss {float(loss):.5f} vs {float(loss_ref):.5f}; "
          f"worst of {len(keys)} gradient tensors {worst[1]:.3e} at {worst[0]}")
    assert e_pred < 2e-2 and abs(float(loss) - float(loss_ref)) < 2e-3 * float(loss_ref)
    assert worst[1] < 8e-2, worst


def test_batch384_bf16_step_on_the_eight_phase_gemm_vs_oracle():
    """A training step large enough for gemm_p8.hip to take the model's big products (batch 384: M = 38400 = 600 tiles of
    256 x 256): its pre-activation copy (F, U), LayerNorm(64) + GELU and GELU' epilogues run in the forward and backward pass.
    Depth 2, G = 512 (the oracle's autograd on the CPU stays in seconds): predictions, loss and every gradient tensor against the
    fp32 oracle at the bf16 tolerances, and against the same step with the kernel switched off (the kernels it replaces)."""
    import ctypes
    _lib.require_gpu()
    lib = _lib.lib()
    cfg = dict(num_outputs=512, input_dim=1024, depth=2, nheads=16, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    sd = vis_oracle.perturb_norm_params(vis_oracle.init_vis_state_dict(**cfg, seed=17), seed=6)
    B = 384                     # 600 tiles: the GELU' epilogue is taken from two full rounds of tiles on
    x = torch.from_numpy(synth.cluster_tokens(5, B, 1024))
    y = torch.from_numpy(synth.rna_targets(8, B, 512))
    torch.set_num_threads(min(32, os.cpu_count()))
    loss_ref, pred_ref, grads_ref = vis_oracle.vis_loss_and_grads(sd, x, y)
    out = {}
    try:
        for on in (1, 0):
            lib.sq_dbg_set(14, on)
            m = ViS(**cfg, device="cuda:0", compute_dtype="bf16")
            m.load_state_dict(sd)
            m.to("cuda:0")
            pred = m._run_forward(x.cuda(), save=True)
            loss, gpred = sq_train.mse_loss_grad(m, pred, y.cuda())
            gflat, _ = sq_train.vis_backward(m, gpred, B, False)
            torch.cuda.synchronize()
            out[on] = (pred.cpu().numpy(), float(loss), {k: v.cpu().numpy() for k, v in m.grad_views(gflat).items()})
    finally:
        lib.sq_dbg_set(14, -1)
    pred, loss, gv = out[1]
    e_pred = rel_err(pred, pred_ref.detach().numpy())
    worst = max(((rel_err(gv[k], grads_ref[k].numpy()), k) for k in grads_ref), key=lambda t: t[0])
    worst_ab = max(((rel_err(gv[k], out[0][2][k]), k) for k in grads_ref), key=lambda t: t[0])
    print(f"B=384 bf16 step on gemm_p8: pred rel err {e_pred:.3e}; loss {loss:.5f} vs {float(loss_ref):.5f}; worst gradient tensor vs oracle "
          f"{worst[0]:.3e} at {worst[1]}, vs the step without the kernel {worst_ab[0]:.3e} at {worst_ab[1]}")
    assert e_pred < 2e-2 and abs(loss - float(loss_ref)) < 2e-3 * float(loss_ref)
    assert worst[0] < 8e-2, worst
    # (measured: bit-equal -- on gfx950 the 16x16x32 and 32x32x16 bf16 MFMAs evidently sum K in the same order; not relied upon)
    assert worst_ab[0] < 5e-2 and rel_err(pred, out[0][0]) < 1e-2


def test_helper_streams_do_not_change_results(monkeypatch):
    """bf16 training step at a realistic size: weight gradients / summary branch on helper streams vs everything on
    one stream must give bit-identical losses and parameters (the kernels are deterministic; streams only reorder)."""
    _lib.require_gpu()
    cfg = dict(num_outputs=1000, input_dim=256, depth=3, nheads=4, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    x = torch.randn(8, 100, 256, generator=torch.Generator().manual_seed(1)).cuda()
    y = (torch.rand(8, 1000, generator=torch.Generator().manual_seed(2)) * 8).cuda()

    def run():
        torch.manual_seed(4)
        m = ViS(**cfg, device="cuda:0", compute_dtype="bf16").to("cuda:0")
        st = sq_train.FusedTrainStep(m, lr=1e-3)
        losses = [float(st.step(x, y)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        return losses, m.flat.detach().clone()

    l_multi, p_multi = run()
    monkeypatch.setenv("SQ_BWD_ONE_STREAM", "1")
    monkeypatch.setenv("SQ_FWD_ONE_STREAM", "1")
    l_one, p_one = run()
    assert l_multi == l_one
    assert torch.equal(p_multi, p_one)


def test_bf16_training_follows_the_fp32_oracle_for_twenty_steps():
    """The bf16 compute mode must TRAIN like the fp32 reference, not only match it for one step: twenty AdamW steps (lr 1e-3,
    weight_decay 0, src/main.py:180-183) of the BASELINE config-2 model on one fixed batch of 32 slides -- the fused HIP step in
    bf16 (bf16 operands and saved activations, fp32 master weights and moments) against CPU fp32 autograd + the restated AdamW
    (oracle/vis_oracle.py).  The loss must stay within 1 % of the reference's at EVERY step."""
    from collections import OrderedDict
    _lib.require_gpu()
    cfg = dict(num_outputs=20820, input_dim=1024, depth=6, nheads=16, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    sd = vis_oracle.perturb_norm_params(vis_oracle.init_vis_state_dict(**cfg, seed=21), seed=3)
    B, steps = 32, 20
    x = torch.from_numpy(synth.cluster_tokens(31, B, 1024))
    y = torch.from_numpy(synth.rna_targets(9, B))
    m = ViS(**cfg, device="cuda:0", compute_dtype="bf16")
    m.load_state_dict(sd)
    m.to("cuda:0")
    st = sq_train.FusedTrainStep(m, lr=1e-3)
    xg, yg = x.cuda(), y.cuda()
    got = [float(st.step(xg, yg)[0]) for _ in range(steps)]
    torch.cuda.synchronize()
    torch.set_num_threads(min(32, os.cpu_count()))
    params = OrderedDict((k, v.clone()) for k, v in sd.items())
    m1 = OrderedDict((k, torch.zeros_like(v)) for k, v in sd.items())
    m2 = OrderedDict((k, torch.zeros_like(v)) for k, v in sd.items())
    ref = []
    for t in range(1, steps + 1):
        loss, _, grads = vis_oracle.vis_loss_and_grads(params, x, y)
        ref.append(float(loss))
        vis_oracle.adamw_step(params, grads, m1, m2, t, lr=1e-3)
    gaps = [abs(a - b) / b for a, b in zip(got, ref)]
    print("20-step trajectory bf16 vs fp32 oracle: loss " + " ".join(f"{a:.4f}/{b:.4f}" for a, b in zip(got[::4], ref[::4])) +
          f"; worst relative gap {max(gaps):.2e} at step {int(np.argmax(gaps)) + 1}")
    assert ref[-1] < 0.9 * ref[0], "the reference itself must be learning on this batch"
    assert max(gaps) < 1e-2, gaps


def test_adamw_per_bucket_is_bit_identical_to_one_pass(monkeypatch):
    """SQ_ADAMW_BUCKETS=1 (opt-in: measured slower on one GPU): every bucket's AdamW update on the communication
    stream as the backward pass completes it -- element-wise, so losses and parameters must equal the one-pass step bit for bit."""
    _lib.require_gpu()
    cfg = dict(num_outputs=500, input_dim=256, depth=3, nheads=4, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    x = torch.randn(8, 100, 256, generator=torch.Generator().manual_seed(11)).cuda()
    y = (torch.rand(8, 500, generator=torch.Generator().manual_seed(12)) * 8).cuda()

    def run():
        torch.manual_seed(5)
        m = ViS(**cfg, device="cuda:0", compute_dtype="bf16").to("cuda:0")
        st = sq_train.FusedTrainStep(m, lr=1e-3)
        losses = [float(st.step(x, y)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        return losses, m.flat.detach().clone(), st

    l0, p0, s0 = run()
    monkeypatch.setenv("SQ_ADAMW_BUCKETS", "1")
    l1, p1, s1 = run()
    assert not s0.adamw_buckets and s1.adamw_buckets and s1.overlap
    assert l0 == l1 and torch.equal(p0, p1)


def test_stream_switch_flipped_between_forward_and_backward_is_an_error_not_garbage(monkeypatch):
    """bf16 mode saves the residual stream in bf16 (lean) or fp32 (SQ_VIS_FP32_STREAM=1) and the backward pass re-reads it: the
    forward pass notes which, and a backward pass that would read the other kind fails loudly."""
    _lib.require_gpu()
    cfg = dict(num_outputs=40, input_dim=128, depth=2, nheads=2, dimensions_f=64, dimensions_s=64, dimensions_c=64)
    torch.manual_seed(3)
    m = ViS(**cfg, device="cuda:0", compute_dtype="bf16").to("cuda:0")
    x = torch.randn(4, 100, 128, device="cuda")
    y = torch.rand(4, 40, device="cuda") * 8
    monkeypatch.delenv("SQ_VIS_FP32_STREAM", raising=False)
    pred = m(x)
    _, g = sq_train.mse_loss_grad(m, pred.detach(), y)
    monkeypatch.setenv("SQ_VIS_FP32_STREAM", "1")
    with pytest.raises(_lib.SequoiaHipError, match="SQ_VIS_FP32_STREAM"):
        pred.backward(g)
    # both passes under one setting: fine either way, and the two settings agree to bf16 accuracy
    grads = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("SQ_VIS_FP32_STREAM", flag)
        m.flat.grad = None
        pred = m(x)
        _, g = sq_train.mse_loss_grad(m, pred.detach(), y)
        pred.backward(g)
        grads[flag] = m.flat.grad.detach().clone()
    assert rel_err(grads["0"].cpu().numpy(), grads["1"].cpu().numpy()) < 3e-2
